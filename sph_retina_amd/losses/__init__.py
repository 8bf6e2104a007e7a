from .sph2pob_iou_loss import (OBBIoULoss, Sph2PobIoULoss, SphIoULoss, SphIoULossLegacy,  # noqa: F401
                               sph2pob_iou_loss)
from .sph2pob_gaussian_loss import (Sph2PobGDLoss, Sph2PobKFLoss, sph2pob_gd_loss,  # noqa: F401
                                    sph2pob_kf_loss)
from .sph2pob_l1_loss import Sph2PobL1Loss  # noqa: F401
from .sph2pob_transform import Sph2PobTransfrom  # noqa: F401
from .focal_loss import FocalLoss, sigmoid_focal_loss, sph_focal_loss  # noqa: F401
from .bbox_loss import sph_bbox_loss  # noqa: F401
from .delta_loss import L1Loss, SmoothL1Loss, sph_delta_loss  # noqa: F401
from .gauss_bbox_loss import sph_gauss_bbox_loss  # noqa: F401
from .point_bbox_loss import sph_point_bbox_loss  # noqa: F401
from .bce_loss import binary_cross_entropy, sph_bce_loss  # noqa: F401
from .softmax_loss import CrossEntropyLoss, cross_entropy, sph_softmax_loss  # noqa: F401
from .rcnn_loss import accuracy, sph_rcnn_bbox_loss, sph_rcnn_loss  # noqa: F401

__all__ = ['Sph2PobIoULoss', 'SphIoULoss', 'OBBIoULoss', 'Sph2PobTransfrom', 'sph2pob_iou_loss', 'Sph2PobL1Loss', 'SphIoULossLegacy',
           'Sph2PobGDLoss', 'Sph2PobKFLoss', 'sph2pob_gd_loss', 'sph2pob_kf_loss', 'FocalLoss', 'sigmoid_focal_loss', 'sph_focal_loss', 'sph_bbox_loss',
           'sph_delta_loss', 'L1Loss', 'SmoothL1Loss', 'sph_gauss_bbox_loss', 'CrossEntropyLoss', 'cross_entropy', 'sph_softmax_loss',
           'sph_point_bbox_loss', 'sph_bce_loss', 'binary_cross_entropy', 'accuracy', 'sph_rcnn_bbox_loss', 'sph_rcnn_loss']

# with mmrotate importable, its GDLoss / KFLoss bodies take the two names over (registry and namespace)
from . import sph2pob_mmrotate_losses as _mm  # noqa: E402
for _name in _mm.__all__:
    globals()[_name] = getattr(_mm, _name)
