"""The fused R-CNN head box loss (`sph_rcnn_bbox_loss`, sph2pob_rcnn_delta_loss_sum_f32 / sph2pob_rcnn_bbox_loss_sum_f32),
`accuracy` and `sph_rcnn_loss`: the scene, a numpy statement of the row rule and the checks that the CPU tier (host twin) and the GPU
tier share — `device` is the only difference between the two.

Yardstick for the arithmetic: the EXISTING flat entries on the gathered rows, `rcnn_bbox_pred` -> `sph_delta_loss` / `sph_bbox_loss`
with the weights of the non-positive rows set to 0.  The new gradient, viewed (S, slots, dim), must have their bits at
[r, label_r] of a positive row and be +0.0 everywhere else; the loss is within 1e-6 relative — the figure `check_layouts` of
bbox_loss_restatement.py uses for "same rows, different span partition": the sums differ in the order of the double partials only.
Yardstick for the row rule: numpy, `0 <= label < C` and the family's weight rule, the L1 elements in float32 and their sum in double.

Shapes: S in {1, 7, 64, 65, 259, 1031} — the run of a wave is 16 rows, four waves per workgroup: a partial only run, exact
multiples, one row beyond a multiple, several workgroups with a partial last one — times (slots, dim) in {(1, 4) class-agnostic,
(3, 5) W = 15: scalar stores, (4, 5) W = 20: 16-byte stores that straddle slots, (37, 4) W = 148: the real row}.
"""
import ctypes
import functools
import math

import numpy as np
import torch

import test_loss_host as TL

ROWS = (1, 7, 64, 65, 259, 1031)
LAYOUTS = ((1, 4), (3, 5), (4, 5), (37, 4))
LAYOUT_IDS = [f'slots{s}-dim{d}' for s, d in LAYOUTS]
MODES = ('iou', 'giou', 'diou', 'ciou')
STDS = (0.1, 0.1, 0.2, 0.2, 0.1)
MAX_RATIO = abs(math.log(16 / 1000))
AGNOSTIC_CLASSES = 3     # classes of the class-agnostic scenes (one slot)
ULP2 = 2.4e-7            # two fp32 ulp, relative
SUM_RTOL = 1e-6          # bbox_loss_restatement.check_layouts: the same rows, summed in another partition of double partials


def coder_of(S, dim):
    cls = S.DeltaXYWHSphBBoxCoder if dim == 4 else S.DeltaXYWHASphBBoxCoder
    return cls(target_means=(0.,) * dim, target_stds=STDS[:dim])


class Scene:
    """float32 / int64 numpy: pred (S, slots dim), labels (S,), deltas (S, dim) encoded targets, boxes (S, dim) decoded targets,
    rois (S, 1 + dim), w_rows (S,), w_elems (S, dim).  Labels: classes, and C (background), -1, C + 5; the first rows hold 0, C - 1,
    C, -1, C + 5 in turn.  Weights: background rows WITH a non-zero weight, positive rows of all-zero and of partial weight."""

    def __init__(self, rows, slots, dim, seed=0):
        rng = np.random.default_rng(1000 * rows + 10 * slots + dim + seed)
        self.rows, self.slots, self.dim = rows, slots, dim
        self.classes = C = slots if slots > 1 else AGNOSTIC_CLASSES
        dead = np.array([C, -1, C + 5])
        labels = np.where(rng.random(rows) < 0.6, rng.integers(0, C, rows), dead[rng.integers(0, 3, rows)])
        first = np.array([0, C - 1, C, -1, C + 5, 0, C - 1])
        labels[:min(rows, 7)] = first[:min(rows, 7)]
        self.labels = labels.astype(np.int64)
        self.pos = (labels >= 0) & (labels < C)
        self.pred = np.ascontiguousarray(rng.standard_normal((rows, slots * dim)) * 0.05, np.float32)
        self.deltas = np.ascontiguousarray(rng.standard_normal((rows, dim)) * 0.05, np.float32)
        box = np.stack([rng.uniform(0, 360, rows), rng.uniform(30, 150, rows), rng.uniform(10, 60, rows), rng.uniform(10, 60, rows),
                        rng.uniform(-40, 40, rows)], 1)[:, :dim]
        self.rois = np.ascontiguousarray(np.concatenate([rng.integers(0, 8, (rows, 1)), box], 1), np.float32)
        t = box + rng.standard_normal((rows, dim)) * np.array([3.0, 3.0, 2.0, 2.0, 4.0])[:dim]
        t[:, 0] %= 360
        self.boxes = np.ascontiguousarray(t, np.float32)
        kind = rng.integers(0, 5, rows)       # 0: zero weight; 1: partial; else ones — on positives and on the others alike
        kind[:min(rows, 7)] = np.array([2, 1, 2, 2, 0, 0, 2])[:min(rows, 7)]
        partial = np.array([1.0, 0.0, 1.0, 0.0, 0.5])[:dim]
        self.w_elems = np.ascontiguousarray(np.where((kind == 0)[:, None], 0.0, np.where((kind == 1)[:, None], partial, 1.0)), np.float32)
        self.w_rows = np.ascontiguousarray(np.where(kind == 0, 0.0, np.where(kind == 1, 0.5, 1.0)), np.float32)

    def weights(self, form):
        return self.w_rows if form == 'rows' else self.w_elems

    def live(self, form, family):
        """The numpy statement of the row rule."""
        w = self.weights(form).reshape(self.rows, -1)
        rule = (w != 0).any(1) if family == 'delta' else (w.astype(np.float64).mean(1) != 0)
        return self.pos & rule

    def slot(self):
        return np.where(self.pos, 0 if self.slots == 1 else self.labels, 0)


@functools.lru_cache(maxsize=None)
def scene(rows, slots, dim, seed=0):
    return Scene(rows, slots, dim, seed)


def t_(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def loss_cfg(family, mode='ciou', beta=0.0, loss_weight=1.0):
    if family == 'delta':
        return dict(type='L1Loss', loss_weight=loss_weight) if beta == 0 else dict(type='SmoothL1Loss', beta=beta, loss_weight=loss_weight)
    return dict(type='Sph2PobIoULoss', mode=mode, loss_weight=loss_weight)


def fused(S, sc, device, family, form='elems', mode='ciou', beta=0.0, grad=True, pred=None, loss_weight=1.0, **kw):
    """(loss, gradient (S, W) | None) of sph_rcnn_bbox_loss on the scene."""
    x = (t_(sc.pred, device) if pred is None else pred).requires_grad_(grad)
    kw.setdefault('reduction', 'sum')
    extra = dict(rois=t_(sc.rois, device), bbox_coder=coder_of(S, sc.dim)) if family == 'bbox' else {}
    targets = t_(sc.deltas if family == 'delta' else sc.boxes, device)
    w = None if form is None else t_(sc.weights(form), device)
    loss = S.sph_rcnn_bbox_loss(x, t_(sc.labels, device), targets, w, num_classes=sc.classes, loss_bbox=loss_cfg(family, mode, beta, loss_weight),
                                reg_class_agnostic=sc.slots == 1, **extra, **kw)
    return loss.detach(), (torch.autograd.grad(loss, x)[0] if grad else None)


def gathered(S, sc, device, family, form='elems', mode='ciou', beta=0.0, zero_dead=True, **kw):
    """The existing flat entry on `rcnn_bbox_pred`'s rows as one flattened level; zero_dead: the weights of the non-positive rows
    set to 0 (without it: what the clamping gather computes when a background row carries a weight)."""
    x = t_(sc.pred, device).requires_grad_(True)
    n, dim = sc.rows, sc.dim
    kw.setdefault('reduction', 'sum')
    picked = S.rcnn_bbox_pred(x, t_(sc.labels, device), sc.classes, dim, sc.slots == 1)
    w = sc.weights(form).reshape(n, -1) * (sc.pos[:, None] if zero_dead else 1.0)
    w = t_(w.astype(np.float32).reshape(sc.weights(form).shape), device)[None]
    if family == 'delta':
        loss = S.sph_delta_loss([picked.view(1, n, dim)], t_(sc.deltas, device)[None], w, beta=beta, **kw)
    else:
        loss = S.sph_bbox_loss([picked.view(1, n, dim)], t_(sc.rois[:, 1:], device), t_(sc.boxes, device)[None], w, bbox_coder=coder_of(S, dim),
                               mode=mode, **kw)
    return loss.detach(), torch.autograd.grad(loss, x)[0]


def assert_selected_slots(sc, g, g_ref, live, what):
    """g (S, W) has g_ref's bits on the live rows' slots and +0.0 with the sign bit clear everywhere else."""
    g3, r3 = g.cpu().view(sc.rows, sc.slots, sc.dim), g_ref.cpu().view(sc.rows, sc.slots, sc.dim)
    r, s = np.nonzero(live)[0], sc.slot()[live]
    assert torch.equal(g3[r, s], r3[r, s]), what
    mask = np.ones((sc.rows, sc.slots), bool)
    mask[r, s] = False
    rest = g3.numpy()[mask]
    assert (rest == 0).all() and not np.signbit(rest).any(), what
    assert np.isfinite(g3.numpy()).all(), what


def close(a, b, what, rtol=SUM_RTOL):
    a, b = float(a), float(b)
    print(f'rcnn loss {what}: {a!r} against {b!r}')
    assert abs(a - b) <= rtol * abs(b), (what, a, b)


# ---- shared checks ----------------------------------------------------------------------------------------------------------
def check_bits_vs_gathered(S, device, rows, slots, dim):
    """Check 1: both weight forms; L1, SmoothL1 and the four IoU modes against the flat entries on the gathered rows."""
    sc = scene(rows, slots, dim)
    for form in ('rows', 'elems'):
        for family, opts in [('delta', dict(beta=0.0)), ('delta', dict(beta=0.04))] + [('bbox', dict(mode=m)) for m in MODES]:
            kw = dict(avg_factor=7.0, reduction='mean')
            loss, g = fused(S, sc, device, family, form, **opts, **kw)
            ref, g_ref = gathered(S, sc, device, family, form, **opts, **kw)
            what = (device, rows, slots, dim, form, family, tuple(opts.values()))
            assert_selected_slots(sc, g, g_ref, sc.live(form, family), what)
            close(loss, ref, what)
            assert float(loss) > 0 or not sc.live(form, family).any(), what


def check_reference_rule(S, device, slots, dim):
    """Check 2: a background row with a non-zero weight adds nothing (numpy gives the sum; the clamping gather would differ), and a
    table without a positive row gives 0 and zeros."""
    sc = scene(259, slots, dim)
    assert (~sc.pos & (sc.w_rows != 0)).any() and (sc.pos & (sc.w_rows == 0)).any()
    for form in ('rows', 'elems'):
        w = sc.weights(form).reshape(sc.rows, -1)
        live = sc.live(form, 'delta')
        r, s = np.nonzero(live)[0], sc.slot()[live]
        picked = sc.pred.reshape(sc.rows, sc.slots, dim)[r, s]
        elems = np.abs(picked - sc.deltas[r]) * np.broadcast_to(w[r], (len(r), dim))     # float32, as the kernel
        want = float(np.float32(elems.astype(np.float64).sum()))
        loss, g = fused(S, sc, device, 'delta', form)
        close(loss, want, (device, 'numpy row rule', slots, dim, form))
        assert bool((g.cpu()[torch.from_numpy(~live)] == 0).all())
        clamped, _ = gathered(S, sc, device, 'delta', form, zero_dead=False)
        assert abs(float(clamped) - want) > 1e-3 * want, 'the scene must tell the reference rule from the clamp'
        for family in ('delta', 'bbox'):
            live = sc.live(form, family)
            _, g = fused(S, sc, device, family, form)
            rowsum = g.cpu().abs().sum(1).numpy()
            assert (rowsum[~live] == 0).all() and (rowsum[live] > 0).mean() > 0.9, (family, form)
    none = Scene(65, slots, dim, seed=5)
    none.labels[:] = np.where(none.pos, none.classes, none.labels)
    none.pos[:] = False
    for family in ('delta', 'bbox'):
        loss, g = fused(S, none, device, family, 'elems')
        assert float(loss) == 0.0 and not np.signbit(float(loss)) and bool((g == 0).all()) and not np.signbit(g.cpu().numpy()).any()


def check_inert(S, device, slots, dim):
    """Check 3: NaN / Inf on every slot of dead rows and on the unselected slots of live rows, NaN in the targets / rois of dead rows
    reach nothing; a NaN in a live row's selected slot reaches the loss and the gradient."""
    sc = scene(259, slots, dim)
    for family in ('delta', 'bbox'):
        live = sc.live('elems', family)
        clean, g_clean = fused(S, sc, device, family)
        dirty = Scene(259, slots, dim)
        p3 = dirty.pred.reshape(sc.rows, sc.slots, dim)
        keep = p3[np.nonzero(live)[0], sc.slot()[live]].copy()
        p3[:] = np.where(np.arange(sc.rows)[:, None, None] % 2 == 0, np.nan, np.inf)
        p3[np.nonzero(live)[0], sc.slot()[live]] = keep
        dirty.deltas[~live] = np.nan
        dirty.boxes[~live] = np.nan
        dirty.rois[~live] = np.nan
        loss, g = fused(S, dirty, device, family)
        assert math.isfinite(float(loss)) and float(loss) == float(clean) and torch.equal(g, g_clean), family
        r0, s0 = np.nonzero(live)[0][0], sc.slot()[live][0]
        p3[r0, s0, 1] = np.nan
        loss, g = fused(S, dirty, device, family)
        assert math.isnan(float(loss)) and bool(torch.isnan(g.view(sc.rows, sc.slots, dim)[r0, s0]).any()), family
        others = torch.ones(sc.rows, dtype=torch.bool)
        others[r0] = False
        assert torch.equal(g.cpu()[others], g_clean.cpu()[others]), family


def cabi(device, sc, family, offset=0, grads=True, mode_code=3, guard=8, **over):
    """One entry through ctypes with the gradient inside a NaN-filled buffer with `guard` floats on both sides and, with `offset`,
    gradient AND input `offset` floats past a 16-byte boundary: (rc, out, gradient view, its buffer)."""
    from sph_retina_amd import _lib
    n, dim, w = sc.rows, sc.dim, sc.slots * sc.dim
    src = torch.zeros((n * w + 16,), device=device)
    pred = src[4 + offset:4 + offset + n * w]
    pred.copy_(t_(sc.pred, device).reshape(-1))
    buf = torch.full((n * w + 2 * guard + 8,), float('nan'), device=device)
    view = buf[guard + offset:guard + offset + n * w]
    assert guard % 4 == 0 and view.data_ptr() % 16 == 4 * offset and pred.data_ptr() % 16 == 4 * offset
    labels, weight = t_(sc.labels, device), t_(sc.w_elems, device)
    need = _lib.lib().sph2pob_rcnn_loss_workspace_bytes(n, sc.slots, dim)
    assert need >= 8
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    out = torch.full((1,), float('nan'), device=device)
    a = dict(pred=pred.data_ptr(), grad=view.data_ptr() if grads else None, rows=n, slots=sc.slots, classes=sc.classes, dim=dim,
             labels=labels.data_ptr(), weight=weight.data_ptr(), wd=dim, scale=1.0, avg=None, out=out.data_ptr(), ws=ws.data_ptr())
    if family == 'delta':
        targets = t_(sc.deltas, device)
        a.update(targets=targets.data_ptr(), beta=0.0)
        a.update(over)
        rc = TL.entry('sph2pob_rcnn_delta_loss_sum_f32', device)(
            a['pred'], a['grad'], a['rows'], a['slots'], a['classes'], a['dim'], a['labels'], a['targets'], a['weight'], a['wd'], a['beta'], a['scale'],
            a['avg'], a['out'], a['ws'], TL.stream(device))
    else:
        targets, rois = t_(sc.boxes, device), t_(sc.rois, device)
        f32s = ctypes.c_float * 5
        a.update(targets=targets.data_ptr(), rois=rois.data_ptr(), stride=1 + dim, off=1, max_ratio=MAX_RATIO, flags=1, mode=mode_code)
        a.update(over)
        rc = TL.entry('sph2pob_rcnn_bbox_loss_sum_f32', device)(
            a['pred'], a['grad'], a['rows'], a['slots'], a['classes'], a['dim'], a['labels'], a['rois'], a['stride'], a['off'], a['targets'], a['weight'],
            a['wd'], f32s(0, 0, 0, 0, 0), f32s(*STDS), a['max_ratio'], a['flags'], 32.0, a['mode'], 1e-6, a['scale'], a['avg'], a['out'], a['ws'],
            TL.stream(device))
    if device != 'cpu':
        torch.cuda.synchronize()
    return rc, out, view, buf


def check_written_once_and_guards(S, device, rows, slots, dim):
    """Check 4, and the offset view of the shape list: every element finite on a NaN-prefilled buffer, the guards intact, aligned and
    one float off alignment (the scalar store path) with the same bits, equal to the Python route; forward only writes nothing."""
    sc = scene(rows, slots, dim)
    guard = 8
    for family in ('delta', 'bbox'):
        ref_loss, ref_g = fused(S, sc, device, family, 'elems')
        for offset in (0, 1):
            rc, out, view, buf = cabi(device, sc, family, offset, guard=guard)
            assert rc == 0, rc
            assert bool(torch.isnan(buf[:guard + offset]).all()) and bool(torch.isnan(buf[guard + offset + view.numel():]).all()), 'guards'
            assert bool(torch.isfinite(view).all()), 'every element of the gradient is written'
            assert float(out) == float(ref_loss) and torch.equal(view.view(ref_g.shape), ref_g), (family, offset)
        rc, out, view, buf = cabi(device, sc, family, 0, grads=False)
        assert rc == 0 and float(out) == float(ref_loss) and bool(torch.isnan(buf).all())


def check_determinism_and_divisors(S, device, slots, dim):
    """Check 5."""
    sc = scene(1031, slots, dim)
    eps = float(torch.finfo(torch.float32).eps)
    for family, elems in (('delta', sc.rows * dim), ('bbox', sc.rows)):
        kw = dict(avg_factor=37.0, reduction='mean', loss_weight=2.0)
        a, ga = fused(S, sc, device, family, **kw)
        b, gb = fused(S, sc, device, family, **kw)
        c, gc = fused(S, sc, device, family, **dict(kw, avg_factor=torch.tensor([37.0], device=device)))
        assert float(a) == float(b) and torch.equal(ga, gb), 'two calls give the same bits'
        assert float(a) == float(c) and torch.equal(ga, gc), 'a device avg_factor gives the bits of the number'
        s, _ = fused(S, sc, device, family)
        m, _ = fused(S, sc, device, family, reduction='mean')
        assert float(a) > 0 and abs(float(a) - 2.0 * float(s) / (37.0 + eps)) <= 1e-6 * float(a)
        assert abs(float(m) - float(s) / elems) <= 1e-6 * float(m)
        try:
            fused(S, sc, device, family, reduction='sum', avg_factor=3.0)
            raise AssertionError('avg_factor with sum must be refused')
        except ValueError:
            pass
        # a second backward through a retained graph recomputes: within one ulp of the first
        x = t_(sc.pred, device).requires_grad_(True)
        extra = dict(rois=t_(sc.rois, device), bbox_coder=coder_of(S, dim)) if family == 'bbox' else {}
        loss = S.sph_rcnn_bbox_loss(x, t_(sc.labels, device), t_(sc.deltas if family == 'delta' else sc.boxes, device), t_(sc.w_elems, device),
                                    num_classes=sc.classes, loss_bbox=loss_cfg(family), reg_class_agnostic=slots == 1, avg_factor=5.0, **extra)
        first = torch.autograd.grad(loss, x, retain_graph=True)[0].clone()
        again = torch.autograd.grad(3.0 * loss, x)[0]
        assert bool(((again - 3.0 * first).abs() <= 3.0 * first.abs() * 2.4e-7).all()) and bool((first != 0).any())
        # no_grad: no stash, no graph
        with torch.no_grad():
            quiet = S.sph_rcnn_bbox_loss(x, t_(sc.labels, device), t_(sc.deltas if family == 'delta' else sc.boxes, device), t_(sc.w_elems, device),
                                         num_classes=sc.classes, loss_bbox=loss_cfg(family), reg_class_agnostic=slots == 1, avg_factor=5.0, **extra)
        assert quiet.grad_fn is None and not quiet.requires_grad and float(quiet) == float(loss.detach())
        # 16-bit inputs are cast; the gradient comes back in their dtype
        for dt in (torch.float16, torch.bfloat16):
            xh = t_(sc.pred, device).to(dt)
            lh, gh = fused(S, sc, device, family, pred=xh.clone(), avg_factor=5.0, reduction='mean')
            lf, gf = fused(S, sc, device, family, pred=xh.float(), avg_factor=5.0, reduction='mean')
            assert gh.dtype is dt and float(lh) == float(lf) and torch.equal(gh, gf.to(dt))


def check_no_grad_allocates_no_stash(S, device):
    from sph_retina_amd.losses import _head as H
    sc = scene(65, 4, 5)
    calls = []
    keep = H.grad_buffer
    H.grad_buffer = lambda *a, **k: calls.append(1) or keep(*a, **k)
    try:
        with torch.no_grad():
            fused(S, sc, device, 'delta', grad=False, pred=t_(sc.pred, device).requires_grad_(True))
        assert not calls
        fused(S, sc, device, 'delta', grad=False)     # a leaf without requires_grad: none either
        assert not calls
        fused(S, sc, device, 'delta')
        assert calls
    finally:
        H.grad_buffer = keep


def check_error_codes(fn_delta, fn_bbox, sc, device):
    """Check 6, the documented codes of one library's two entries, in the documented order; nothing is enqueued."""
    NULL, DIM, OPTION, SIZE = -1, -2, -3, -4
    f32s = ctypes.c_float * 5
    pred, labels, targets, rois, w = (t_(a, device) for a in (sc.pred, sc.labels, sc.deltas, sc.rois, sc.w_elems))
    out, ws = torch.zeros(1, device=device), torch.zeros(64, device=device)
    n, dim, slots, C = sc.rows, sc.dim, sc.slots, sc.classes

    def delta(**o):
        a = dict(pred=pred.data_ptr(), rows=n, slots=slots, classes=C, dim=dim, labels=labels.data_ptr(), targets=targets.data_ptr(),
                 weight=w.data_ptr(), wd=dim, beta=0.0, out=out.data_ptr(), ws=ws.data_ptr())
        a.update(o)
        return fn_delta(a['pred'], None, a['rows'], a['slots'], a['classes'], a['dim'], a['labels'], a['targets'], a['weight'], a['wd'], a['beta'], 1.0,
                        None, a['out'], a['ws'], None)

    def bbox(**o):
        a = dict(pred=pred.data_ptr(), rows=n, slots=slots, classes=C, dim=dim, labels=labels.data_ptr(), rois=rois.data_ptr(), stride=1 + dim, off=1,
                 targets=targets.data_ptr(), weight=w.data_ptr(), wd=dim, max_ratio=MAX_RATIO, flags=1, mode=3, out=out.data_ptr(), ws=ws.data_ptr())
        a.update(o)
        return fn_bbox(a['pred'], None, a['rows'], a['slots'], a['classes'], a['dim'], a['labels'], a['rois'], a['stride'], a['off'], a['targets'],
                       a['weight'], a['wd'], f32s(0, 0, 0, 0, 0), f32s(*STDS), a['max_ratio'], a['flags'], 32.0, a['mode'], 1e-6, 1.0, None, a['out'],
                       a['ws'], None)

    for fn in (delta, bbox):
        assert fn(dim=3) == DIM and fn(dim=6) == DIM
        assert fn(wd=2) == OPTION
        assert fn(classes=0) == OPTION and fn(slots=0) == OPTION and fn(slots=C + 1) == OPTION and fn(slots=2, classes=5) == OPTION
        assert fn(rows=-1) == SIZE
        assert fn(slots=4097, classes=4097, dim=5, wd=5) == SIZE and fn(slots=5121, classes=5121, dim=4, wd=4) == SIZE   # slots * dim > 4096 * 5
        assert fn(rows=(1 << 31) // (slots * dim), pred=None) == SIZE                                           # rows * W beyond 32-bit indices
        assert fn(out=None) == NULL and fn(ws=None) == NULL and fn(pred=None) == NULL and fn(labels=None) == NULL and fn(targets=None) == NULL
        assert fn(dim=3, wd=2, rows=-1, out=None) == DIM and fn(wd=2, rows=-1, out=None) == OPTION and fn(rows=-1, out=None) == SIZE   # the order
    assert delta(beta=-1.0) == OPTION and delta(beta=float('nan')) == OPTION
    assert bbox(mode=4) == OPTION and bbox(mode=3 | 0x200) == OPTION and bbox(flags=4) == OPTION and bbox(max_ratio=-1.0) == OPTION
    assert bbox(stride=dim, off=1) == SIZE and bbox(off=-1) == SIZE and bbox(rois=None) == NULL


def check_python_errors(S, device):
    import pytest
    sc = scene(65, 4, 5)
    x, lab, tg, w, rois = (t_(a, device) for a in (sc.pred, sc.labels, sc.deltas, sc.w_elems, sc.rois))
    coder = coder_of(S, 5)
    kw = dict(num_classes=4)
    with pytest.raises(ValueError, match='bbox_pred must be'):
        S.sph_rcnn_bbox_loss(x[:, :15], lab, tg, w, **kw)
    with pytest.raises(ValueError, match='bbox_pred must be'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, num_classes=4, reg_class_agnostic=True)
    with pytest.raises(ValueError, match='labels must be'):
        S.sph_rcnn_bbox_loss(x, lab[:-1], tg, w, **kw)
    with pytest.raises(ValueError, match='labels must be'):
        S.sph_rcnn_bbox_loss(x, lab.float(), tg, w, **kw)
    with pytest.raises(ValueError, match='bbox_targets must be'):
        S.sph_rcnn_bbox_loss(x, lab, tg[:, :3], w, **kw)
    with pytest.raises(ValueError, match='bbox_weights must be'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w[:, :2], **kw)
    with pytest.raises(ValueError, match='num_classes'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, num_classes=0)
    with pytest.raises(ValueError, match='reduced scalar'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, reduction='none', **kw)
    with pytest.raises(ValueError, match="'mean' or 'sum'"):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, reduction='max', **kw)
    iou = dict(type='Sph2PobIoULoss', mode='giou')
    with pytest.raises(ValueError, match='rois and bbox_coder'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=iou, bbox_coder=coder, **kw)
    with pytest.raises(ValueError, match='rois and bbox_coder'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=iou, rois=rois, **kw)
    with pytest.raises(ValueError, match='rois must be'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=iou, rois=rois[:, :4], bbox_coder=coder, **kw)
    with pytest.raises(ValueError, match='4-component coder|component coder'):
        S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=iou, rois=rois, bbox_coder=coder_of(S, 4), **kw)
    with pytest.raises(RuntimeError, match='one device|MI355X'):
        S.sph_rcnn_bbox_loss(x, lab.to('meta'), tg, w, **kw)
    import sph_retina_amd.losses as L
    for bad in (dict(type='Sph2PobGDLoss', loss_type='kld'), dict(type='Sph2PobKFLoss'), dict(type='Sph2PobL1Loss'), dict(type='GDLoss'),
                dict(type='RotatedIoULoss'), L.Sph2PobL1Loss(), L.Sph2PobGDLoss(loss_type='gwd'), L.SphIoULoss(), torch.nn.L1Loss()):
        with pytest.raises(NotImplementedError, match='rcnn_bbox_pred'):
            S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=bad, rois=rois, bbox_coder=coder, **kw)
    # instances are taken as they are: beta and loss_weight are read
    a = S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=S.SmoothL1Loss(beta=0.04, loss_weight=3.0), avg_factor=5.0, **kw)
    b = S.sph_rcnn_bbox_loss(x, lab, tg, w, loss_bbox=dict(type='SmoothL1Loss', beta=0.04, loss_weight=3.0), avg_factor=5.0, **kw)
    assert float(a) == float(b) and float(a) > 0
    # plain (S, dim) rois are the table's rois without the image index
    c = S.sph_rcnn_bbox_loss(x, lab, t_(sc.boxes, device), w, loss_bbox=S.Sph2PobIoULoss(mode='giou'), rois=rois, bbox_coder=coder, **kw)
    d = S.sph_rcnn_bbox_loss(x, lab, t_(sc.boxes, device), w, loss_bbox=iou, rois=rois[:, 1:], bbox_coder=coder, **kw)
    assert float(c) == float(d) and float(c) > 0


def check_empty(S, device):
    for dim in (4, 5):
        x = torch.zeros((0, 3 * dim), device=device, requires_grad=True)
        args = (x, torch.zeros((0,), dtype=torch.int64, device=device), torch.zeros((0, dim), device=device), None)
        for extra in (dict(), dict(loss_bbox=dict(type='Sph2PobIoULoss'), rois=torch.zeros((0, 1 + dim), device=device), bbox_coder=coder_of(S, dim))):
            s = S.sph_rcnn_bbox_loss(*args, num_classes=3, reduction='sum', **extra)
            assert float(s.detach()) == 0.0 and torch.autograd.grad(s, x)[0].shape == x.shape
            assert torch.isnan(S.sph_rcnn_bbox_loss(*args, num_classes=3, reduction='mean', **extra))
            assert float(S.sph_rcnn_bbox_loss(*args, num_classes=3, avg_factor=3.0, **extra)) == 0.0


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def mmdet_accuracy(pred, target, topk=1, thresh=None):
    """mmdet/models/losses/accuracy.py:7-48, stated directly (tie-free logits: the rank of the target's score)."""
    single = isinstance(topk, int)
    ks = (topk,) if single else topk
    score = pred.gather(1, target.view(-1, 1))
    rank = (pred > score).sum(1)                     # 0: the target is the top score
    res = []
    for k in ks:
        hit = rank < k
        if thresh is not None:
            hit = hit & (score.view(-1) > thresh)
        res.append(hit.float().sum(0, keepdim=True).mul_(100.0 / pred.size(0)))
    return res[0] if single else res


def check_accuracy(S, device):
    g = torch.Generator().manual_seed(11)
    n, k, pad = 203, 9, 53
    pred = torch.randn((n, k), generator=g).to(device)
    target = torch.randint(0, k, (n,), generator=g).to(device)
    target[::3] = pred[::3].argmax(1)                # a third certainly right
    for topk in (1, (1, 5)):
        for thresh in (None, 0.5):
            got, want = S.accuracy(pred, target, topk, thresh), mmdet_accuracy(pred, target, topk, thresh)
            got, want = ([got], [want]) if isinstance(topk, int) else (got, want)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.shape == b.shape == (1,) and torch.equal(a, b) and 0 < float(a) < 100, (topk, thresh)
            # a padded table: rows of weight 0 in between and behind; the divisor is the count of the real rows
            rows = torch.randperm(n + pad, generator=g)[:n].sort().values.to(device)
            p2 = torch.randn((n + pad, k), generator=g).to(device)
            t2 = p2.argmax(1)                         # the padding rows would all count as hits
            w2 = torch.zeros(n + pad, device=device)
            p2[rows], t2[rows], w2[rows] = pred, target, 1.0
            for avg in (float(n), n, torch.tensor(float(n), device=device)):
                padded = S.accuracy(p2, t2, topk, thresh, weight=w2, avg_factor=avg)
                padded = [padded] if isinstance(topk, int) else padded
                for a, b in zip(padded, want):   # a device divisor: count * 100 / n rounded once, mmdet count * (100.0 / n): 2 ulp apart at most
                    assert torch.equal(a, b) if not torch.is_tensor(avg) else torch.allclose(a, b, rtol=ULP2, atol=0), (topk, thresh, avg)
    zero = S.accuracy(pred, target, weight=torch.zeros(n, device=device), avg_factor=torch.tensor(0.0, device=device))
    assert float(zero) == 0.0
    assert float(S.accuracy(pred[:0], target[:0])) == 0.0
    assert float(S.accuracy(pred, target, avg_factor=0)) >= 0


# ---- the head's loss() on a table --------------------------------------------------------------------------------------------
def rcnn_table(S, device, decoded, seed=4242):
    """The scene of check 8: B = 3, num = 16, M = 40, C = 5, image 1 without GT -> (targets, coder, C)."""
    import rcnn_targets_restatement as RT
    proposals, gts, labs = RT.to(device, *RT.draw(4, seed=9, m=40, num_proposals=(40, 33, 40), gt_counts=(4, 0, 3)))
    labs = [l % 5 for l in labs]
    cfg = RT.rcnn_cfg('sph2pob_standard_iou', 4, num=16, neg_iou_thr=0.3)
    coder = coder_of(S, 4)
    n_dev = torch.tensor((40, 33, 40), dtype=torch.int64, device=device)
    # concatenated GT with offsets: the list form builds its offsets with a host-to-device copy, which a capture does not take
    gt, lab, off = torch.cat(gts), torch.cat(labs), torch.tensor((0, 4, 4, 7), dtype=torch.int64).to(device)

    def targets(s):
        return S.sph_rcnn_targets(proposals, gt, lab, off, num_proposals=n_dev, train_cfg=cfg, num_classes=5, seed=s, reg_decoded_bbox=decoded,
                                  bbox_coder=coder, k_max=4)
    return targets, coder, 5


def head_loss(S, t, cls_score, bbox_pred, coder, C, decoded):
    kw = dict(loss_bbox=dict(type='Sph2PobIoULoss', mode='iou'), reg_decoded_bbox=True) if decoded else {}
    return S.sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=C, bbox_coder=coder, **kw)


def demo_composition(S, t, cls_score, bbox_pred, coder, C, decoded):
    """tools/demo_hot_path.py::run_rcnn_batch._rcnn_losses as it composes the two losses today."""
    loss_cls = S.cross_entropy(cls_score, t.labels, t.label_weights, avg_factor=t.avg_factor)
    picked = S.rcnn_bbox_pred(bbox_pred, t.labels, C, 4, False)
    if decoded:
        loss_box = S.Sph2PobIoULoss(mode='iou', loss_weight=1.0)(coder.decode(t.rois[:, 1:].contiguous(), picked), t.bbox_targets, t.bbox_weights,
                                                                 avg_factor=t.num_samples)
    else:
        loss_box = S.L1Loss(loss_weight=1.0)(picked, t.bbox_targets, t.bbox_weights, avg_factor=t.num_samples)
    return loss_cls, loss_box


def check_head_loss(S, device, decoded):
    """sph_rcnn_loss on a real table against today's composition: loss_cls and its gradient are the same node; loss_bbox and its
    gradient under the rule of check 1 against the flat entry on the gathered rows (for L1 that IS the composition: L1Loss is
    sph_delta_loss on one flattened level).  The decoded composition, coder.decode -> Sph2PobIoULoss, runs the same per-box
    functions in two kernels with an fp32 tree sum: it is held the way bbox_loss_restatement.check_clip_and_ratio_gate holds
    fused against composition — the same zero pattern, 4 ulp per element, 1e-5 on the sum."""
    targets, coder, C = rcnn_table(S, device, decoded)
    t = targets(4242)
    n = t.labels.size(0)
    assert n == 48 and int(t.num_pos[1]) == 0 and int(t.num_pos.sum()) > 0
    g = torch.Generator().manual_seed(2)
    cls_score = torch.randn((n, C + 1), generator=g).to(device).requires_grad_(True)
    bbox_pred = (torch.randn((n, C * 4), generator=g) * 0.05).to(device).requires_grad_(True)
    out = head_loss(S, t, cls_score, bbox_pred, coder, C, decoded)
    assert set(out) == {'loss_cls', 'acc', 'loss_bbox'}
    g_cls, g_box = torch.autograd.grad(out['loss_cls'] + out['loss_bbox'], (cls_score, bbox_pred))
    c_cls, c_box = demo_composition(S, t, cls_score, bbox_pred, coder, C, decoded)
    cg_cls, cg_box = torch.autograd.grad(c_cls + c_box, (cls_score, bbox_pred))
    assert torch.equal(out['loss_cls'], c_cls) and torch.equal(g_cls, cg_cls)
    live = t.label_weights != 0
    want_acc = mmdet_accuracy(cls_score[live], t.labels[live])
    assert torch.allclose(out['acc'], want_acc, rtol=ULP2, atol=0) and 0 < float(want_acc) < 100     # the divisor is the device count
    pos = ((t.labels >= 0) & (t.labels < C)).cpu().numpy()
    picked = S.rcnn_bbox_pred(bbox_pred, t.labels, C, 4, False)
    if decoded:
        flat = S.sph_bbox_loss([picked.view(1, n, 4)], t.rois[:, 1:].contiguous(), t.bbox_targets[None], t.bbox_weights[None], bbox_coder=coder,
                               mode='iou', avg_factor=t.num_samples)
    else:
        flat = S.sph_delta_loss([picked.view(1, n, 4)], t.bbox_targets[None], t.bbox_weights[None], avg_factor=t.num_samples)
    fg_box = torch.autograd.grad(flat, bbox_pred)[0]
    assert bool((t.bbox_weights[torch.from_numpy(~pos).to(device)] == 0).all())     # the table's own weights: dead rows carry none
    assert torch.equal(g_box, fg_box) and bool((g_box != 0).any())
    close(out['loss_bbox'].detach(), flat.detach(), (device, 'head loss_bbox vs flat entry', decoded))
    if decoded:
        eps32 = float(np.finfo(np.float32).eps)
        assert torch.equal(g_box == 0, cg_box == 0) and bool(((g_box - cg_box).abs() <= 4 * eps32 * cg_box.abs()).all())
        close(out['loss_bbox'].detach(), c_box.detach(), (device, 'head loss_bbox vs decode -> Sph2PobIoULoss'), rtol=1e-5)
    else:
        assert torch.equal(g_box, cg_box)
        close(out['loss_bbox'].detach(), c_box.detach(), (device, 'head loss_bbox vs L1Loss on the gather'))
    import pytest
    with pytest.raises(ValueError, match='reg_decoded_bbox=True'):
        S.sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=C, bbox_coder=coder, loss_bbox=dict(type='Sph2PobIoULoss'))
    with pytest.raises(NotImplementedError, match='rcnn_bbox_pred'):
        S.sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=C, bbox_coder=coder, reg_decoded_bbox=True)
    with pytest.raises(NotImplementedError, match='CrossEntropyLoss'):
        S.sph_rcnn_loss(cls_score, bbox_pred, t, num_classes=C, bbox_coder=coder, loss_cls=dict(type='FocalLoss'))


# ---- device against host twin, and the captured step (GPU tier) ---------------------------------------------------------------
def check_device_equals_twin_delta(S, rows, slots, dim):
    """As test_gpu_delta_loss.py holds its pair: the same element function in both libraries — gradients bit for bit, the loss
    within 1e-6 (the partials are composed differently)."""
    sc = scene(rows, slots, dim)
    for form in ('rows', 'elems'):
        for beta in (0.0, 0.04):
            (ld, gd), (lh, gh) = (fused(S, sc, d, 'delta', form, beta=beta, avg_factor=7.0, reduction='mean') for d in ('cuda', 'cpu'))
            assert torch.equal(gd.cpu(), gh), (rows, slots, dim, form, beta)
            close(ld, lh, ('delta device vs twin', rows, slots, dim, form, beta))


def check_device_equals_twin_decoded(S, box, mode):
    """As test_gpu_bbox_loss.py::test_device_equals_host_twin holds ITS pair, on its scene: the positives of
    bbox_loss_restatement.main_scene as the rows of a table (random classes, the anchors as rois), |device - twin| in the statistics
    and scales of that file's f64 side, within test_loss_host.BOUNDS[(box, 'near', mode)] — the two libraries' expf / sincosf /
    atan2f differ, so not bit for bit."""
    import bbox_loss_restatement as BR
    bsc, ref = BR.main_scene(box), BR.f64_side('main', box, mode)
    gb, _, vb = TL.BOUNDS[(box, 'near', mode)]
    b, i = ref['b'], ref['i']
    n, dim, C = len(b), bsc.dim, 4
    rng = np.random.default_rng(5)
    labels = rng.integers(0, C, n)
    pred = np.ascontiguousarray(rng.standard_normal((n, C, dim)) * 0.05, np.float32)
    pred[np.arange(n), labels] = bsc.deltas[b, i]
    rois = np.ascontiguousarray(np.concatenate([b[:, None].astype(np.float32), bsc.anchors[i]], 1), np.float32)
    coder = BR.coder_of(S, dim)

    def run(device, w, grad):
        x = t_(pred.reshape(n, C * dim), device).requires_grad_(grad)
        loss = S.sph_rcnn_bbox_loss(x, t_(labels.astype(np.int64), device), t_(bsc.targets[b, i], device), w, num_classes=C, rois=t_(rois, device),
                                    bbox_coder=coder, loss_bbox=dict(type='Sph2PobIoULoss', mode=mode), reduction='sum')
        return loss.detach(), (torch.autograd.grad(loss, x)[0].view(n, C, dim)[torch.arange(n), torch.from_numpy(labels)].cpu().numpy() if grad else None)

    def values(device):
        out, w = np.zeros(n, np.float32), torch.zeros(n, device=device)
        for j in range(n):
            w[j] = 1.0
            out[j] = float(run(device, w, False)[0])
            w[j] = 0.0
        return out
    (ld, gd), (lh, gh) = run('cuda', None, True), run('cpu', None, True)
    d = (gd.astype(np.float64) - gh)[ref['smooth']][:, ~ref['zero']] / ref['scale'][~ref['zero']]
    gs = TL.three(np.abs(d))
    vs = TL.three(np.abs(values('cuda').astype(np.float64) - values('cpu')))
    print(f'rcnn bbox loss device vs host {box} {mode}: gradient {gs} value {vs} sums {float(ld)!r} {float(lh)!r} bit-equal grads {bool((gd == gh).all())}')
    TL.within(gs, gb, (box, mode, 'gradient'))
    TL.within(vs, vb, (box, mode, 'value'))
    assert abs(float(ld) - float(lh)) <= n * vb[1]


def check_captured_step(S, decoded):
    """Check 8: sph_rcnn_targets -> sph_rcnn_loss -> autograd.grad wrt cls_score and bbox_pred, captured with the default queue
    setting; two replays with changed head outputs and a changed device seed equal the eager step bit for bit."""
    targets, coder, C = rcnn_table(S, 'cuda', decoded)
    n = 48
    cls_score = torch.zeros((n, C + 1), device='cuda', requires_grad=True)
    bbox_pred = torch.zeros((n, C * 4), device='cuda', requires_grad=True)
    seed = torch.tensor(40, dtype=torch.int64, device='cuda')

    def step(s):
        t = targets(s)
        out = head_loss(S, t, cls_score, bbox_pred, coder, C, decoded)
        return (out['loss_cls'], out['acc'], out['loss_bbox']) + torch.autograd.grad(out['loss_cls'] + out['loss_bbox'], (cls_score, bbox_pred)) + (
            t.labels, t.num_pos)

    def load(k):
        gg = torch.Generator().manual_seed(k)
        with torch.no_grad():
            cls_score.copy_(torch.randn(cls_score.shape, generator=gg))
            bbox_pred.copy_(torch.randn(bbox_pred.shape, generator=gg) * 0.05)
    load(20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(seed)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(seed)
    labels = []
    for k in (21, 22):
        load(k)
        seed += 1
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step(int(seed))
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert torch.isfinite(got[0]) and float(got[0]) > 0 and float(got[2]) > 0 and int(got[-1].sum()) > 0 and int(got[-1][1]) == 0
        assert bool((got[3] != 0).any()) and bool((got[4] != 0).any()) and bool(torch.isfinite(got[4]).all())
        labels.append(got[-2])
    assert not torch.equal(labels[0], labels[1])     # the device seed was re-read
