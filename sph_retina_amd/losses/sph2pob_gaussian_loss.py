"""`Sph2PobGDLoss` / `Sph2PobKFLoss` — the reference's Gaussian losses (sphdet/losses/sph2pob_gd_loss.py,
sph2pob_kf_loss.py: mmrotate's `GDLoss` / `KFLoss` behind the `Sph2PobTransfrom` decorator), fused end to end like
`Sph2PobIoULoss`:

    forward : ONE kernel  (jitter -> sph2pob_standard -> jitter -> Gaussian body -> x weight)
              + the deterministic two-pass sum for 'mean' / 'sum'
    backward: ONE kernel  (closed-form adjoint of the body, the shared chain rule down to the spherical inputs), or with
              a gradient in sight the one-pass forward + gradient stash that torch's backward only scales

The bodies are mmrotate 0.3.2's `gaussian_dist_loss.py` (gwd / kld / jd / kld_symmax / kld_symmin with the `postprocess`
map) and `kf_iou_loss.py`, restated from the published source: mmrotate is absent here, so parity with it is UNPINNED
(as for `SphIoULossLegacy`).  The tests hold the kernels to a float64 matrix-form restatement of those bodies.
Differences from mmrotate:
- the all-zero-weight shortcut (`torch.any(weight > 0)`) needs a device->host sync; here zero weights give a zero loss
  with zero gradients on the normal path (as in `Sph2PobIoULoss`);
- KFIoU's covariance `S_T - S_T (S_T + S_P)^-1 S_T` has its determinant in closed form, always positive: where
  mmrotate's fp32 matrix inverse makes it negative (NaN volume, counted as 0, NaN gradients) this gives the exact value.
When mmrotate IS importable, `sph2pob_mmrotate_losses` builds both names from mmrotate's own classes and they take
precedence (registry and package namespace).
"""
import torch.nn as nn

from .. import _torch_glue as G
from ..registry import LOSSES
from .sph2pob_iou_loss import GAUSS_FAMILY, weighted_loss_apply

GD_LOSS_TYPES = {'gwd': 0, 'kld': 1, 'jd': 2, 'kld_symmax': 3, 'kld_symmin': 4}
KF_TYPE = 5
GD_FUNS = {'none': 0, 'log1p': 1, 'sqrt': 2}
KF_FUNS = {'none': 0, 'ln': 3, 'exp': 4}
OPT_SQRT, OPT_NORMALIZE = 1, 2
# keyword arguments each mmrotate loss function accepts besides (fun, tau, alpha) / the decode boxes
_GD_KWARGS = {'gwd': ('normalize',), 'kld': ('sqrt',), 'jd': ('sqrt',), 'kld_symmax': ('sqrt',), 'kld_symmin': ('sqrt',)}
_KF_KWARGS = ('beta', 'eps')


def _type_code(code):
    """loss type | arithmetic flag (reference-order front end when set_arithmetic('reference') is active)."""
    return code | (G.FLAG_REFERENCE_ORDER if G.get_arithmetic() == 'reference' else 0)


def _check_kwargs(kwargs, allowed, fn):
    for k in kwargs:
        if k not in allowed:
            raise TypeError(f"{fn}() got an unexpected keyword argument '{k}'")


def _checked_weight(weight, pred):
    """An (n, box_dim) weight must match pred (mmrotate asserts it).  mmrotate then takes `weight.mean(-1)` after
    Sph2PobTransfrom widened an (n, 4) weight with its mean: the kernels take that same per-box mean (weight_dim = box_dim)."""
    if weight is not None and weight.dim() > 1:
        assert weight.shape == pred.shape
    return weight


def sph2pob_gd_loss(pred, target, weight=None, loss_type='kld', fun='log1p', tau=0.0, alpha=1.0, sqrt=True,
                    normalize=True, reduction='mean', avg_factor=None, loss_weight=1.0):
    """Functional form: loss_weight * weight_reduce_loss(<loss_type>_loss(sph2pob(pred, target)), weight, ...)."""
    assert loss_type in GD_LOSS_TYPES and fun in GD_FUNS
    opts = (OPT_SQRT if sqrt else 0) | (OPT_NORMALIZE if normalize else 0)
    tail = (_type_code(GD_LOSS_TYPES[loss_type]), GD_FUNS[fun], float(tau), float(alpha), opts, 0.0, 0.0)
    return weighted_loss_apply(pred, target, weight, GAUSS_FAMILY, tail, reduction, avg_factor, loss_weight)


def sph2pob_kf_loss(pred, target, weight=None, fun='none', beta=1.0 / 9.0, eps=1e-6, reduction='mean', avg_factor=None,
                    loss_weight=1.0):
    """Functional form: loss_weight * weight_reduce_loss(kfiou_loss(sph2pob(pred, target)), weight, ...)."""
    assert fun in KF_FUNS
    tail = (_type_code(KF_TYPE), KF_FUNS[fun], 0.0, 1.0, 0, float(beta), float(eps))
    return weighted_loss_apply(pred, target, weight, GAUSS_FAMILY, tail, reduction, avg_factor, loss_weight)


@LOSSES.register_module(force=True)
class Sph2PobGDLoss(nn.Module):
    """dict(type='Sph2PobGDLoss', loss_type='kld', ...) — mmrotate's GDLoss on the Sph2Pob planar boxes.

    loss_type: 'gwd' | 'kld' | 'jd' | 'kld_symmax' | 'kld_symmin'; fun: 'log1p' | 'none' | 'sqrt'.  `sqrt` (kld family,
    default True) and `normalize` (gwd, default True) arrive through **kwargs, from the constructor or from `forward`.
    `tau` defaults to 0.0 as mmrotate's code has it (its docstring says 1.0).  Only `representation='xy_wh_r'` exists:
    the transform produces (x, y, w, h, a) boxes."""

    def __init__(self, loss_type, representation='xy_wh_r', fun='log1p', tau=0.0, alpha=1.0, reduction='mean',
                 loss_weight=1.0, **kwargs):
        super().__init__()
        assert reduction in ['none', 'sum', 'mean']
        assert fun in ['log1p', 'none', 'sqrt']
        assert loss_type in GD_LOSS_TYPES
        if representation != 'xy_wh_r':
            raise ValueError(f"representation {representation!r}: the Sph2Pob transform produces 'xy_wh_r' boxes only")
        self.loss_type = loss_type
        self.representation = representation
        self.fun = fun
        self.tau = tau
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.kwargs = kwargs

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        _kwargs = dict(self.kwargs)
        _kwargs.update(kwargs)
        _check_kwargs(_kwargs, _GD_KWARGS[self.loss_type], f'{self.loss_type}_loss')
        return sph2pob_gd_loss(pred, target, _checked_weight(weight, pred), loss_type=self.loss_type, fun=self.fun,
                               tau=self.tau, alpha=self.alpha, sqrt=_kwargs.get('sqrt', True),
                               normalize=_kwargs.get('normalize', True), reduction=reduction, avg_factor=avg_factor,
                               loss_weight=self.loss_weight)


@LOSSES.register_module(force=True)
class Sph2PobKFLoss(nn.Module):
    """dict(type='Sph2PobKFLoss', fun='none') — mmrotate's KFLoss on the Sph2Pob planar boxes, with the reference's
    swapped decode boxes (pred_decode = planar target, targets_decode = planar pred).  fun: 'none' | 'ln' | 'exp';
    `forward` also takes beta (1/9, smooth-L1 of the centres) and eps (1e-6).  Constructor **kwargs are ignored, as
    in mmrotate."""

    def __init__(self, fun='none', reduction='mean', loss_weight=1.0, **kwargs):
        super().__init__()
        assert fun in ['none', 'ln', 'exp']
        self.fun = fun
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        _check_kwargs(kwargs, _KF_KWARGS, 'kfiou_loss')
        return sph2pob_kf_loss(pred, target, _checked_weight(weight, pred), fun=self.fun, beta=kwargs.get('beta', 1.0 / 9.0),
                               eps=kwargs.get('eps', 1e-6), reduction=reduction, avg_factor=avg_factor,
                               loss_weight=self.loss_weight)
