from .get_bboxes import DetBBoxes, sph_get_bboxes, sph_test_bboxes  # noqa: F401
from .softmax_bboxes import sph_softmax_bboxes, sph_softmax_scores  # noqa: F401
from .fcos_bboxes import sph_fcos_bboxes  # noqa: F401
from .rcnn_bboxes import sph_rcnn_bboxes  # noqa: F401
from .sph_nms import PlanarNMS, SphNMS, sph_batched_nms, sph_nms_op  # noqa: F401
from .utils import multiclass_nms  # noqa: F401

__all__ = ['PlanarNMS', 'SphNMS', 'sph_batched_nms', 'sph_nms_op', 'multiclass_nms', 'sph_get_bboxes', 'sph_test_bboxes', 'DetBBoxes', 'sph_softmax_bboxes',
           'sph_softmax_scores', 'sph_fcos_bboxes', 'sph_rcnn_bboxes']
