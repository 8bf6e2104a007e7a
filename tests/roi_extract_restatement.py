"""The yardstick of sph_roi_extract: the scenes, and the reference's box transform (sphdet/models/heads/sph_rcnn_head.py:211-230),
the level rule of SingleRoIExtractor.map_roi_levels and mmcv-full 1.6.0's RoIAlign ('avg') restated in numpy.

The position arithmetic — the box, the level, the sampling frame, every sample's indices and weights — is np.float32 in the order
the C header states; the sums are float64.  Because the bilinear weights are separable, a roi's outputs are Wy F Wx^T with Wy
(PH, H) and Wx (PW, W) holding the fp32 weights of the valid samples: every product and sum of that is float64.  Besides the value
the restatement returns what the tests' bounds need: per output `count` and A, the same sum over |feat|; per feature pixel of the
backward the number of terms T and the sum of their absolute values.
"""
import numpy as np

F32 = np.float32
IMG = (64, 128)                       # img_h, img_w
STRIDES = (4, 8, 16, 32)              # maps 16x32, 8x16, 4x8, 2x4
FINEST = 8
B = 3
COUNTS = (29, 0, 17)
M = 32
DEG = 2.8125                          # degrees per pixel on both axes of the 64 x 128 image (45 / 16: exact)
U24 = 2.0 ** -24


def level_shapes(strides=STRIDES, img=IMG):
    return [(img[0] // s, img[1] // s) for s in strides]


def make_feats(channels, strides=STRIDES, seed=0):
    rng = np.random.default_rng(100 + seed)
    return [rng.standard_normal((B, channels, h, w)).astype(F32) for h, w in level_shapes(strides)]


# ---- rois ----

def _px(cx, cy, w, h, g=None):
    """A roi given in pixels of the image -> degrees."""
    r = [cx * DEG, cy * DEG, w * DEG, h * DEG]
    return r + ([g] if g is not None else [])


def handmade(dim):
    """The hand-made rois (module docstring of tests/test_roi_extract_host.py names each)."""
    g = (lambda v: v) if dim == 5 else (lambda v: None)
    t = 1.0 if dim == 4 else 1.1      # dim 5: off the level thresholds (the device's sine and cosine are not torch's)
    rois = [
        _px(40, 30, 0, 0, g(20.0)),            # zero extent
        _px(64, 32, 128, 64, g(0.0)),          # the whole image
        _px(64, 20, 128, 2 * t, g(0.0)),       # a 128 x 2 px sliver (dim 4: scale 16, on the threshold of level 1)
        _px(64, 40, 128, 0.4, g(0.0)),         # thinner: level 0, gw = 5 with gh = 1
        _px(30, 32, 0.9, 64, g(0.0)),          # the upright one: level 0, gh = 3
        _px(50.3, 20.6, 0.3, 0.3, g(33.0)),    # sub-pixel: all bins in one cell
        _px(2, 30, 12, 9, g(-15.0)),           # over the theta = 0 seam
        _px(127, 12, 10, 14, g(70.0)),         # over the right border
        _px(70, 1.5, 20, 8, g(5.0)),           # over the top
        _px(33, 63, 9, 11, g(-80.0)),          # over the bottom: y_low >= H - 1
        _px(0, 0, 30, 30, g(45.0)),            # a corner
        _px(128, 64, 6, 6, g(10.0)),           # the opposite corner, centre on the border
    ]
    rois += [_px(64, 32, 8 * t * 2 ** k, 8 * t * 2 ** k, g(0.0 if dim == 4 else 12.0 * k)) for k in range(5)]   # level thresholds
    return np.asarray(rois, dtype=F32)


THRESHOLD_ROWS = slice(12, 17)
THRESHOLD_LEVELS = [0, 1, 2, 3, 3]


def _scale_f64(box, dim, img=IMG):
    xy = transform_f64(box, dim, img)
    return np.sqrt((xy[:, 2] - xy[:, 0]) * (xy[:, 3] - xy[:, 1]))


def away_from_thresholds(box, dim, finest=FINEST, levels=len(STRIDES), rel=1e-3):
    t = _scale_f64(box, dim) / finest + 1e-6
    return np.all([np.abs(t / 2.0 ** k - 1.0) >= rel for k in range(1, levels)], axis=0)


def random_rois(dim, n=40, seed=0):
    rng = np.random.default_rng(7 + seed + 10 * dim)
    out = []
    while len(out) < n:
        r = [rng.uniform(0, 360), rng.uniform(5, 175), np.exp(rng.uniform(np.log(1.0), np.log(200.0))), np.exp(rng.uniform(np.log(1.0), np.log(150.0)))]
        if dim == 5:
            r.append(rng.uniform(-90, 90))
        r = np.asarray([r], dtype=F32)
        if dim == 4 or away_from_thresholds(r, dim)[0]:
            out.append(r[0])
    return np.asarray(out, dtype=F32)


def valid_rois(dim, seed=0):
    """(boxes (n, dim), image index (n,)): the hand-made rois first, then the random ones; images 0 and 2 in the COUNTS proportion."""
    box = np.concatenate([handmade(dim), random_rois(dim, seed=seed)])
    img = np.where(np.arange(len(box)) < COUNTS[0], 0, 2)
    img[COUNTS[0] + COUNTS[2]:] = np.arange(len(box) - COUNTS[0] - COUNTS[2]) % B   # the rest: any image (the flat form only)
    return box, img.astype(np.int64)


REFUSED_INDEX = [-1.0, float(B), 0.5, float('nan')]


def flat_scene(dim, seed=0):
    """The reference's flat table: every valid roi, then the refused rows — image index -1, B, 0.5, NaN; a NaN, +inf, -inf box
    component — in a shuffled order.  Returns (rois (N, 1 + dim), ok (N,) bool)."""
    box, img = valid_rois(dim, seed)
    rows = [np.concatenate([[i], b]) for i, b in zip(img, box)]
    ok = [True] * len(rows)
    for bad in REFUSED_INDEX:
        rows.append(np.concatenate([[bad], box[6]]))
    for k, bad in ((1, np.nan), (3, np.inf), (2, -np.inf), (dim, np.nan)):
        r = np.concatenate([[2.0], box[7]])
        r[k] = bad
        rows.append(r)
    ok += [False] * (len(rows) - len(ok))
    perm = np.random.default_rng(3 + seed).permutation(len(rows))
    return np.asarray(rows, dtype=F32)[perm], np.asarray(ok)[perm]


def padded_scene(dim, seed=0, garbage=np.nan):
    """The padded form: (B, M, dim + 1) with a score column behind the box, counts COUNTS, `garbage` behind the counts.
    Returns (rois, num_rois int64, ok (B * M,) bool)."""
    box, _ = valid_rois(dim, seed)
    rois = np.full((B, M, dim + 1), garbage, dtype=F32)
    ok = np.zeros((B, M), dtype=bool)
    at = 0
    for b, n in enumerate(COUNTS):
        rois[b, :n, :dim] = box[at:at + n]
        rois[b, :n, dim] = 0.5
        ok[b, :n] = True
        at += n
    return rois, np.asarray(COUNTS, dtype=np.int64), ok.reshape(-1)


def rows_of(rois, num_rois, dim):
    """(image (R,), box (R, dim), live (R,)) of either form, flattened; live: in front of the count (flat: every row)."""
    if rois.ndim == 2:
        return rois[:, 0].copy(), rois[:, 1:1 + dim], np.ones(len(rois), dtype=bool)
    b, m = rois.shape[:2]
    n = np.clip(np.asarray(num_rois) if num_rois is not None else np.full(b, m), 0, m)
    live = (np.arange(m)[None, :] < n[:, None]).reshape(-1)
    return np.repeat(np.arange(b), m).astype(F32), rois[..., :dim].reshape(b * m, -1), live


# ---- the box ----

def transform(box, dim, img=IMG):
    """fp32, the header's order: (n, 4) planar boxes clamped to the image."""
    box = np.asarray(box, dtype=F32)
    ih, iw = F32(img[0]), F32(img[1])
    x = box[:, 0] / F32(360) * iw
    y = box[:, 1] / F32(180) * ih
    w = box[:, 2] / F32(360) * iw
    h = box[:, 3] / F32(180) * ih
    if dim == 5:
        a = box[:, 4] * F32(np.pi / 180)
        ca, sa = np.abs(np.cos(a)), np.abs(np.sin(a))
        w, h = ca * w + sa * h, sa * w + ca * h
    x1, y1, x2, y2 = x - w / F32(2), y - h / F32(2), x + w / F32(2), y + h / F32(2)
    out = np.stack([np.clip(x1, F32(0), iw), np.clip(y1, F32(0), ih), np.clip(x2, F32(0), iw), np.clip(y2, F32(0), ih)], axis=1)
    assert out.dtype == F32
    return out


def transform_f64(box, dim, img=IMG):
    box = np.asarray(box, dtype=np.float64)
    ih, iw = float(img[0]), float(img[1])
    x, y, w, h = box[:, 0] / 360 * iw, box[:, 1] / 180 * ih, box[:, 2] / 360 * iw, box[:, 3] / 180 * ih
    if dim == 5:
        a = np.deg2rad(box[:, 4])
        ca, sa = np.abs(np.cos(a)), np.abs(np.sin(a))
        w, h = ca * w + sa * h, sa * w + ca * h
    return np.stack([np.clip(x - w / 2, 0, iw), np.clip(y - h / 2, 0, ih), np.clip(x + w / 2, 0, iw), np.clip(y + h / 2, 0, ih)], axis=1)


def transform_torch(box, dim, img=IMG):
    """The reference's expressions in fp32 torch (what its own evaluation of the formula gives on these rois)."""
    import torch
    r = torch.from_numpy(np.asarray(box, dtype=F32))
    ih, iw = img
    t, p, al, be = torch.chunk(r[:, :4], 4, dim=1)
    b = torch.cat([(t / 360) * iw, (p / 180) * ih, (al / 360) * iw, (be / 180) * ih], dim=1)
    if dim == 5:
        a = r[:, 4].deg2rad()
        ca, sa = torch.cos(a).abs(), torch.sin(a).abs()
        b = torch.stack((b[:, 0], b[:, 1], ca * b[:, 2] + sa * b[:, 3], sa * b[:, 2] + ca * b[:, 3]), -1)
    x, y, w, h = torch.chunk(b, 4, dim=1)
    b = torch.cat([x - w / 2, y - h / 2, x + w / 2, y + h / 2], dim=1)
    b[:, [1, 3]] = b[:, [1, 3]].clamp(min=0, max=ih)
    b[:, [0, 2]] = b[:, [0, 2]].clamp(min=0, max=iw)
    return b.numpy()


def levels_of(xyxy, finest=FINEST, num_levels=len(STRIDES)):
    """The count rule: #{k in 1 .. L-1: fl32(scale / finest + 1e-6) >= 2^k}."""
    xyxy = np.asarray(xyxy, dtype=F32)
    with np.errstate(invalid='ignore'):
        scale = np.sqrt((xyxy[:, 2] - xyxy[:, 0]) * (xyxy[:, 3] - xyxy[:, 1]))
        t = scale / F32(finest) + F32(1e-6)
        assert t.dtype == F32
        return sum((t >= F32(2.0 ** k)).astype(np.int32) for k in range(1, num_levels)) + np.zeros(len(xyxy), dtype=np.int32)


def levels_torch(xyxy, finest=FINEST, num_levels=len(STRIDES)):
    """map_roi_levels verbatim (single_level_roi_extractor.py:36-55)."""
    import torch
    rois = torch.from_numpy(np.concatenate([np.zeros((len(xyxy), 1), dtype=F32), np.asarray(xyxy, dtype=F32)], axis=1))
    scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
    lvls = torch.floor(torch.log2(scale / finest + 1e-6))
    return lvls.clamp(min=0, max=num_levels - 1).long().numpy()


def refused(image, box, live, num_images=B):
    """Rows that hold zeros: behind the count, an image index that is no integer of [0, B), a non-finite box component."""
    with np.errstate(invalid='ignore'):
        idx_ok = (image >= 0) & (image < num_images) & (image == np.floor(image))
    return ~live | ~idx_ok | ~np.isfinite(box).all(axis=1)


# ---- RoIAlign ----

def _axis(start, bin_size, g, bins, n):
    """(weights (bins, n) f64, term counts (bins, n)) of one axis: sample i of bin q at start + q bin + (i + .5) bin / g, fp32."""
    W, T = np.zeros((bins, n)), np.zeros((bins, n))
    if g <= 0:
        return W, T
    q = np.repeat(np.arange(bins), g).astype(F32)
    i = np.tile(np.arange(g), bins).astype(F32)
    y = (start + q * bin_size) + ((i + F32(0.5)) * bin_size) / F32(g)
    assert y.dtype == F32
    valid = (y >= F32(-1)) & (y <= F32(n))
    y = np.where(y <= 0, F32(0), y)
    lo = y.astype(np.int64)
    top = lo >= n - 1
    lo = np.where(top, n - 1, lo)
    hi = np.where(top, n - 1, lo + 1)
    y = np.where(top, lo.astype(F32), y)
    ly = y - lo.astype(F32)
    hy = F32(1) - ly
    assert ly.dtype == F32 and hy.dtype == F32
    for k in np.nonzero(valid)[0]:
        b = int(q[k])
        W[b, lo[k]] += float(hy[k]); T[b, lo[k]] += 1
        W[b, hi[k]] += float(ly[k]); T[b, hi[k]] += 1
    return W, T


def frame(xyxy_row, stride, ph, pw, ratio, aligned):
    """(sw, sh, bin_w, bin_h, gw, gh) of a roi on its level, fp32."""
    s, off = F32(1.0 / stride), F32(0.5 if aligned else 0.0)
    x1, y1, x2, y2 = (F32(v) for v in xyxy_row)
    sw, sh, ew, eh = x1 * s - off, y1 * s - off, x2 * s - off, y2 * s - off
    rw, rh = ew - sw, eh - sh
    if not aligned:
        rw, rh = max(rw, F32(1)), max(rh, F32(1))
    bin_h, bin_w = rh / F32(ph), rw / F32(pw)
    gh = ratio if ratio > 0 else int(np.ceil(rh / F32(ph)))
    gw = ratio if ratio > 0 else int(np.ceil(rw / F32(pw)))
    for v in (sw, sh, bin_w, bin_h):
        assert isinstance(v, F32)
    return sw, sh, bin_w, bin_h, max(gw, 0), max(gh, 0)


class Align:
    """RoIAlign of all rows on given planar boxes and levels: forward values with their bounds' ingredients, and the adjoint."""

    def __init__(self, feats, image, xyxy, levels, zero, strides=STRIDES, output_size=(7, 7), ratio=0, aligned=True):
        self.feats = [np.asarray(f, dtype=np.float64) for f in feats]
        self.ph, self.pw = output_size
        self.rows = []
        for r in range(len(xyxy)):
            if zero[r]:
                self.rows.append(None)
                continue
            lvl = int(levels[r])
            h, w = self.feats[lvl].shape[2:]
            sw, sh, bin_w, bin_h, gw, gh = frame(xyxy[r], strides[lvl], self.ph, self.pw, ratio, aligned)
            Wy, Ty = _axis(sh, bin_h, gh, self.ph, h)
            Wx, Tx = _axis(sw, bin_w, gw, self.pw, w)
            self.rows.append((int(image[r]), lvl, Wy, Wx, Ty, Tx, max(gh * gw, 1), (gh, gw)))

    def forward(self):
        """(out (R, C, PH, PW) f64, count (R,), A (R, C, PH, PW))."""
        C = self.feats[0].shape[1]
        out = np.zeros((len(self.rows), C, self.ph, self.pw))
        A = np.zeros_like(out)
        count = np.ones(len(self.rows))
        for r, row in enumerate(self.rows):
            if row is None:
                continue
            b, lvl, Wy, Wx, _, _, cnt, _ = row
            f = self.feats[lvl][b]
            out[r] = np.einsum('ph,chw,qw->cpq', Wy, f, Wx) / cnt
            A[r] = np.einsum('ph,chw,qw->cpq', Wy, np.abs(f), Wx) / cnt
            count[r] = cnt
        return out, count, A

    def backward(self, grad_out):
        """(grads per level f64, T per level (B, H, W): the terms a pixel of ANY channel receives, S per level: sum of |terms|)."""
        go = np.asarray(grad_out, dtype=np.float64)
        grads = [np.zeros_like(f) for f in self.feats]
        S = [np.zeros_like(f) for f in self.feats]
        T = [np.zeros((f.shape[0],) + f.shape[2:]) for f in self.feats]
        for r, row in enumerate(self.rows):
            if row is None:
                continue
            b, lvl, Wy, Wx, Ty, Tx, cnt, _ = row
            grads[lvl][b] += np.einsum('ph,cpq,qw->chw', Wy, go[r] / cnt, Wx)
            S[lvl][b] += np.einsum('ph,cpq,qw->chw', Wy, np.abs(go[r]) / cnt, Wx)
            T[lvl][b] += np.einsum('ph,qw->hw', Ty, Tx)
        return grads, T, S


def forward_bound(count, A):
    """(count + 8) 2^-24 A: the gamma-bound of four products, `count` additions and one division."""
    return (count[:, None, None, None] + 8) * U24 * A


def backward_bound(T, S):
    """(T + 4) 2^-24 sum|terms| per pixel."""
    return [(t[:, None] + 4) * U24 * s for t, s in zip(T, S)]
