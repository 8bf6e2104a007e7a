"""sph_retina_amd — MI355X-native Sph2Pob spherical-IoU engine (drop-in for the reference's sphdet.iou /
sphdet.losses / sphdet.bbox.nms operator surface; kernels in csrc/, C ABI in include/sph2pob_hip.h)."""
from . import _lib  # noqa: F401
from ._torch_glue import get_arithmetic, set_arithmetic  # noqa: F401
from .iou import (SphOverlaps2D, sph2pob_efficient_iou, sph2pob_legacy_iou, sph2pob_standard_iou,  # noqa: F401
                  sph_overlaps)

from .losses import (CrossEntropyLoss, FocalLoss, L1Loss, SmoothL1Loss, Sph2PobIoULoss, SphIoULoss, binary_cross_entropy, cross_entropy,  # noqa: F401,E402
                     sigmoid_focal_loss, sph_bbox_loss, sph_delta_loss, sph_focal_loss, sph_bce_loss, sph_gauss_bbox_loss,
                     sph_point_bbox_loss, sph_softmax_loss, accuracy, sph_rcnn_bbox_loss, sph_rcnn_loss)
from .bbox.nms import (DetBBoxes, SphNMS, multiclass_nms, sph_fcos_bboxes, sph_get_bboxes, sph_rcnn_bboxes, sph_softmax_bboxes,  # noqa: F401,E402
                       sph_softmax_scores, sph_test_bboxes)
from .bbox.assigners import (AnchorTargets, PointTargets, RcnnTargets, SphMaxIoUAssigner, rcnn_bbox_pred, sph_anchor_targets,  # noqa: F401,E402
                             sph_fcos_points, sph_fcos_targets, sph_rcnn_targets, sph_rpn_targets, sph_sample_targets, sph_train_targets)
from .bbox.roi_extract import RoIFeats, SphSingleRoIExtractor, sph_roi_extract  # noqa: F401,E402
from .bbox.coder import DeltaXYWHASphBBoxCoder, DeltaXYWHSphBBoxCoder, DistancePointSphBBoxCoder  # noqa: F401,E402

__version__ = '0.1.0'
