from .delta_sph_bbox_coder import (DeltaXYWHASphBBoxCoder, DeltaXYWHSphBBoxCoder, bbox2delta,  # noqa: F401
                                   delta2bbox)
from .distance_point_sph_bbox_coder import DistancePointSphBBoxCoder, bbox2distance, distance2bbox  # noqa: F401

__all__ = ['DeltaXYWHSphBBoxCoder', 'DeltaXYWHASphBBoxCoder', 'bbox2delta', 'delta2bbox', 'DistancePointSphBBoxCoder', 'bbox2distance',
           'distance2bbox']
