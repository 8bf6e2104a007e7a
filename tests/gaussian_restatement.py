"""The Gaussian losses' yardstick: a plain torch float64 restatement of mmrotate 0.3.2's gaussian_dist_loss.py and
kf_iou_loss.py bodies, written matrix-style as mmrotate writes them (bmm, det, inverse) — not the kernels' closed forms.
Inputs are planar (x, y, w, h, a[rad]) boxes; every function is differentiable by torch autograd."""
import torch


def xy_sigma(b):
    xy = b[:, :2]
    wh = b[:, 2:4].clamp(min=1e-7, max=1e7)
    r = b[:, 4]
    R = torch.stack((torch.cos(r), -torch.sin(r), torch.sin(r), torch.cos(r)), dim=-1).reshape(-1, 2, 2)
    S = 0.5 * torch.diag_embed(wh)
    return xy, R.bmm(S.square()).bmm(R.permute(0, 2, 1))


def postprocess(d, fun='log1p', tau=1.0):
    if fun == 'log1p':
        d = torch.log1p(d)
    elif fun == 'sqrt':
        d = torch.sqrt(d.clamp(1e-7))
    elif fun != 'none':
        raise ValueError(fun)
    return 1 - 1 / (tau + d) if tau >= 1.0 else d


def gwd(p, t, fun='log1p', tau=1.0, alpha=1.0, normalize=True):
    (xy_p, S_p), (xy_t, S_t) = xy_sigma(p), xy_sigma(t)
    xy = (xy_p - xy_t).square().sum(-1)
    whr = S_p.diagonal(dim1=-2, dim2=-1).sum(-1) + S_t.diagonal(dim1=-2, dim2=-1).sum(-1)
    tr = S_p.bmm(S_t).diagonal(dim1=-2, dim2=-1).sum(-1)
    det_sqrt = (S_p.det() * S_t.det()).clamp(1e-7).sqrt()
    whr = whr + (-2) * (tr + 2 * det_sqrt).clamp(1e-7).sqrt()
    d = (xy + alpha * alpha * whr).clamp(1e-7).sqrt()
    if normalize:
        d = d / (2 * det_sqrt.clamp(1e-7).sqrt().clamp(1e-7).sqrt().clamp(1e-7))
    return postprocess(d, fun, tau)


def kld(p, t, fun='log1p', tau=1.0, alpha=1.0, sqrt=True):
    (xy_p, S_p), (xy_t, S_t) = xy_sigma(p), xy_sigma(t)
    S_p_inv = torch.stack((S_p[..., 1, 1], -S_p[..., 0, 1], -S_p[..., 1, 0], S_p[..., 0, 0]), dim=-1).reshape(-1, 2, 2)
    S_p_inv = S_p_inv / S_p.det().unsqueeze(-1).unsqueeze(-1)
    dxy = (xy_p - xy_t).unsqueeze(-1)
    xy = 0.5 * dxy.permute(0, 2, 1).bmm(S_p_inv).bmm(dxy).view(-1)
    whr = 0.5 * S_p_inv.bmm(S_t).diagonal(dim1=-2, dim2=-1).sum(-1)
    whr = whr + 0.5 * (S_p.det().log() - S_t.det().log()) - 1
    d = xy / (alpha * alpha) + whr
    if sqrt:
        d = d.clamp(1e-7).sqrt()
    return postprocess(d, fun, tau)


def jd(p, t, fun='log1p', tau=1.0, alpha=1.0, sqrt=True):
    d = 0.5 * (kld(p, t, 'none', 0, alpha, False) + kld(t, p, 'none', 0, alpha, False))
    if sqrt:
        d = d.clamp(1e-7).sqrt()
    return postprocess(d, fun, tau)


def kld_symmax(p, t, fun='log1p', tau=1.0, alpha=1.0, sqrt=True):
    return postprocess(torch.max(kld(p, t, 'none', 0, alpha, sqrt), kld(t, p, 'none', 0, alpha, sqrt)), fun, tau)


def kld_symmin(p, t, fun='log1p', tau=1.0, alpha=1.0, sqrt=True):
    return postprocess(torch.min(kld(p, t, 'none', 0, alpha, sqrt), kld(t, p, 'none', 0, alpha, sqrt)), fun, tau)


GD = {'gwd': gwd, 'kld': kld, 'jd': jd, 'kld_symmax': kld_symmax, 'kld_symmin': kld_symmin}


def gd(p, t, loss_type, fun='log1p', tau=0.0, alpha=1.0, **kw):
    return GD[loss_type](p, t, fun=fun, tau=tau, alpha=alpha, **kw)


def kfiou(pred, target, pred_decode, targets_decode, fun='none', beta=1.0 / 9.0, eps=1e-6):
    _, S_p = xy_sigma(pred_decode)
    _, S_t = xy_sigma(targets_decode)
    diff = torch.abs(pred[:, :2] - target[:, :2])
    xy = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta).sum(-1)
    Vb_p = 4 * S_p.det().sqrt()
    Vb_t = 4 * S_t.det().sqrt()
    K = S_p.bmm((S_p + S_t).inverse())
    S = S_p - K.bmm(S_p)
    Vb = 4 * S.det().sqrt()
    Vb = torch.where(torch.isnan(Vb), torch.full_like(Vb, 0), Vb)
    k = Vb / (Vb_p + Vb_t - Vb + eps)
    if fun == 'ln':
        kf = -torch.log(k + eps)
    elif fun == 'exp':
        kf = torch.exp(1 - k) - 1
    else:
        kf = 1 - k
    return (xy + kf).clamp(0)


def kf(p, t, fun='none', beta=1.0 / 9.0, eps=1e-6):
    """Sph2PobKFLoss's call: pred_decode = planar target, targets_decode = planar pred."""
    return kfiou(p, t, t, p, fun=fun, beta=beta, eps=eps)
