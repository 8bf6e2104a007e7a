"""The box-regression loss of `SphRetinaHead.loss_single` with `reg_decoded_bbox=True` and a Gaussian `loss_bbox`
(`Sph2PobGDLoss`: gwd / kld / jd / kld_symmax / kld_symmin, or `Sph2PobKFLoss`) as ONE fused pass — `sph_bbox_loss` with the
Gaussian body in place of the IoU family:

    sph_gauss_bbox_loss(bbox_preds, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder,
                        loss=dict(type='Sph2PobGDLoss', loss_type='kld', fun='log1p', tau=1.0), avg_factor=t.avg_factor)

Per positive the arithmetic is the composition's (csrc/sph2pob_coder.hpp decode_one, csrc/sph2pob_loss.hpp pair_gauss_loss).  The
layouts, the weight forms, the zero-weight rule (such a row is never read: exact zero loss, exact +0.0 gradient, a NaN there stays
inert), the deterministic sum, the device-tensor `avg_factor` and the native 16-bit levels are those of `sph_bbox_loss`, whose
autograd node this function shares.  No gradient flows into anchors, targets, weights or `avg_factor`.
"""
from . import _head as H
from . import sph2pob_gaussian_loss as GL
from .bbox_loss import decoded_loss_apply

_NATIVE = ('Sph2PobGDLoss', 'Sph2PobKFLoss')


def _is_native(cls):
    """One of the two classes of sph2pob_gaussian_loss (not mmrotate's, which take the names over in the registry when importable)."""
    return isinstance(cls, type) and cls.__module__ == GL.__name__ and cls.__name__ in _NATIVE


def _loss_module(loss):
    """The package's own Sph2PobGDLoss / Sph2PobKFLoss: `loss` itself, or built from its cfg dict."""
    if isinstance(loss, dict):
        cfg = dict(loss)
        cls = cfg.pop('type', None)
        if isinstance(cls, str) and cls in _NATIVE:
            cls = getattr(GL, cls)
        if not _is_native(cls):
            raise TypeError(f"loss: type must be 'Sph2PobGDLoss' or 'Sph2PobKFLoss', got {loss.get('type')!r}")
        return cls(**cfg)
    if _is_native(type(loss)):
        return loss
    raise TypeError(f'loss must be a Sph2PobGDLoss / Sph2PobKFLoss of this package or the cfg dict of one, got {type(loss).__name__}')


def _gauss_tail(module, kwargs):
    """(type_flags, fun, tau, alpha, opts, beta, eps) of the entry, with the keywords merged and checked as `forward` does."""
    if type(module).__name__ == 'Sph2PobKFLoss':
        GL._check_kwargs(kwargs, GL._KF_KWARGS, 'kfiou_loss')
        return (GL._type_code(GL.KF_TYPE), GL.KF_FUNS[module.fun], 0.0, 1.0, 0, float(kwargs.get('beta', 1.0 / 9.0)),
                float(kwargs.get('eps', 1e-6)))
    merged = dict(module.kwargs)
    merged.update(kwargs)
    GL._check_kwargs(merged, GL._GD_KWARGS[module.loss_type], f'{module.loss_type}_loss')
    opts = (GL.OPT_SQRT if merged.get('sqrt', True) else 0) | (GL.OPT_NORMALIZE if merged.get('normalize', True) else 0)
    return (GL._type_code(GL.GD_LOSS_TYPES[module.loss_type]), GL.GD_FUNS[module.fun], float(module.tau), float(module.alpha), opts, 0.0, 0.0)


def sph_gauss_bbox_loss(bbox_preds, anchors, bbox_targets, bbox_weights=None, *, bbox_coder, loss, avg_factor=None,
                        reduction_override=None, **kwargs):
    """The Gaussian regression loss of a whole minibatch from the head's own outputs, as one scalar.

    bbox_preds, anchors, bbox_targets, bbox_weights, bbox_coder and avg_factor exactly as for `sph_bbox_loss`.  loss: a
    Sph2PobGDLoss / Sph2PobKFLoss of this package or the cfg dict that builds one; its loss_type, fun, tau, alpha, reduction,
    loss_weight and stored kwargs are read.  **kwargs: the forward keywords of those modules (`sqrt`, `normalize`; `beta`, `eps`),
    merged and checked as `forward` does.  Equals loss(coder.decode(anchors repeated, cat of the permuted levels), targets, weights,
    avg_factor=..., **kwargs) without the copies and without the work on the rows of weight 0; the gradient arrives at each
    bbox_preds[l] in its own layout (one autograd node with L inputs).  'mean' without avg_factor divides by B n."""
    module = _loss_module(loss)
    assert reduction_override in (None, 'none', 'mean', 'sum')
    reduction = reduction_override if reduction_override else module.reduction
    H.check_reduction('sph_gauss_bbox_loss', reduction,
                      f"for the loss of every box use {type(module).__name__}(reduction='none') on bbox_coder.decode(...)")
    tail = _gauss_tail(module, kwargs)
    return decoded_loss_apply('sph_gauss_bbox_loss', 'gauss_bbox_loss', tail, bbox_preds, anchors, bbox_targets, bbox_weights, bbox_coder,
                              reduction, avg_factor, module.loss_weight)
