from .max_iou_assigner import AssignResult, SphMaxIoUAssigner, assign_wrt_overlaps, fused_assign  # noqa: F401
from .anchor_targets import AnchorTargets, sph_anchor_targets  # noqa: F401
from .train_targets import sph_train_targets  # noqa: F401
from .sample_targets import sph_rpn_targets, sph_sample_targets  # noqa: F401
from .point_targets import PointTargets, sph_fcos_points, sph_fcos_targets  # noqa: F401
from .rcnn_targets import RcnnTargets, rcnn_bbox_pred, sph_rcnn_targets  # noqa: F401

__all__ = ['SphMaxIoUAssigner', 'AssignResult', 'assign_wrt_overlaps', 'fused_assign', 'AnchorTargets', 'sph_anchor_targets', 'sph_train_targets', 'sph_sample_targets',
           'sph_rpn_targets', 'PointTargets', 'sph_fcos_points', 'sph_fcos_targets', 'RcnnTargets', 'rcnn_bbox_pred', 'sph_rcnn_targets']
