"""Shared by tests/test_softmax_bboxes_host.py and tests/test_gpu_softmax_bboxes.py (a helper: it holds no test): the scenes of a
softmax head (K = C + 1 logits per anchor, the background last), the float64 yardstick of its foreground probabilities and the
derived bound between the two.

The yardstick is `torch.softmax(logits.double(), -1)[..., :-1]` on the logits the kernel reads (fp32, or 16-bit widened),
rearranged to the layout `sph_softmax_scores` writes: (B, A C, H, W) for NCHW levels, (B, n, C) for flat ones."""
import torch

A, C = 3, 8                              # scene S: K = 9, odd — an anchor's channel group straddles the 4-wide loads
S_SHAPES = ((23, 31), (8, 16))           # H W = 713 (no multiple of 4; A C H W = 17 112 > one 16 384-score chunk) and 128 (the vector path)
S_IMAGES = 4
S_ZERO_IMAGE = 1
SMALL = dict(nms_pre=300, max_per_img=60)
FIELDS = ('dets', 'labels', 'prior_inds', 'num_dets')
SSD300_SHAPES = ((38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1))
SSD300_ANCHORS = (4, 6, 6, 6, 4, 4)      # 8 732 anchors


def bound(D):
    """Relative error of an fp32 probability against the f64 softmax of the same logits: (5 + 2 D) 2^-24, D the largest
    |x_j - m| of the scene (the derivation is in test_probabilities_against_f64's docstring)."""
    return (5 + 2 * D) * 2.0 ** -24


def spread(levels, K):
    """D: the largest |x_j - m| over every row of every level (NCHW or flat)."""
    d = 0.0
    for t in levels:
        rows = rows_of(t.double(), K)
        d = max(d, float((rows.max(-1).values[..., None] - rows).max()))
    return d


def rows_of(t, K):
    """(B, A K, H, W) -> (B, A, H, W, K) view-like copy; (B, n, K) as it is: the classes of a row along the last axis."""
    if t.dim() == 4:
        b, ak, h, w = t.shape
        return t.reshape(b, ak // K, K, h, w).permute(0, 1, 3, 4, 2)
    return t


def f64_probs(t, K):
    """The yardstick for one level, in float64, in the layout sph_softmax_scores writes."""
    p = torch.softmax(rows_of(t.double(), K), -1)[..., :-1]
    if t.dim() == 4:
        b, ak, h, w = t.shape
        return p.permute(0, 1, 4, 2, 3).reshape(b, ak // K * (K - 1), h, w)
    return p


def to_flat(t, per_anchor):
    """The head's NCHW (B, A per_anchor, H, W) -> the reference's flat (B, H W A, per_anchor)."""
    b, ap, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b, h * w * (ap // per_anchor), per_anchor).contiguous()


def anchors_for(shapes, per_position, dim, g, device):
    out = []
    for (h, w), a in zip(shapes, per_position):
        u = torch.rand((h * w * a, 5), generator=g)
        out.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim]
                   .contiguous().to(device))
    return out


def head_logits(images, shapes, per_position, num_classes, dim, g, device, zero_image=None, fg=(0.0, 2.0), bg=2.0):
    """NCHW logits and deltas of a softmax head.  Foreground logits N(fg) clamped to +-4.5 around their mean, the background at
    `bg`; image `zero_image` has its background 20 above its largest foreground logit (every foreground probability < 3e-9);
    then every anchor's K logits are shifted together by a uniform draw from +-90, so that a softmax without the max subtraction
    overflows.  |x_j - m| <= 9 + 20 everywhere: no probability is subnormal."""
    K = num_classes + 1
    cls, box = [], []
    for (h, w), a in zip(shapes, per_position):
        x = (torch.randn((images, a, K, h, w), generator=g) * fg[1]).clamp(-4.5, 4.5) + fg[0]
        x[:, :, -1] = bg
        if zero_image is not None:
            x[zero_image, :, -1] = x[zero_image, :, :-1].max(1).values + 20
        x = x + (torch.rand((images, a, 1, h, w), generator=g) * 2 - 1) * 90
        cls.append(x.reshape(images, a * K, h, w).contiguous().to(device))
        box.append((torch.randn((images, a * dim, h, w), generator=g) * 0.5).to(device))
    return cls, box


def scene_s(dim=4, layout='nchw', device='cpu', seed=0, images=S_IMAGES, zero_image=S_ZERO_IMAGE):
    """Scene S -> (logits, deltas, anchors), two levels, in the NCHW or the flat layout."""
    g = torch.Generator().manual_seed(seed)
    anchors = anchors_for(S_SHAPES, (A, A), dim, g, device)
    cls, box = head_logits(images, S_SHAPES, (A, A), C, dim, g, device, zero_image=zero_image)
    if layout == 'flat':
        cls, box = [to_flat(t, C + 1) for t in cls], [to_flat(t, dim) for t in box]
    return cls, box, anchors


def ssd300_scene(device='cpu', seed=0, images=2, num_classes=37):
    """SSD300's six levels (8 732 anchors), K = 38, BFoV: a sparse head — the foreground N(-3, 2) under a background at 0."""
    g = torch.Generator().manual_seed(seed)
    anchors = anchors_for(SSD300_SHAPES, SSD300_ANCHORS, 4, g, device)
    cls, box = head_logits(images, SSD300_SHAPES, SSD300_ANCHORS, num_classes, 4, g, device, fg=(-3.0, 2.0), bg=0.0)
    return cls, box, anchors


def decisive_scene(layout='nchw', device='cpu', seed=0, images=S_IMAGES):
    """Scene S's anchor counts (20 184 candidates per image) with probabilities that leave no doubt: per image
    linspace(0.002, 0.11, 20 184) in f64 shuffled over (anchor, class), background = 1 - row sum (>= 0.12),
    logits = log p + shift, shift uniform in +-60 per anchor, cast to fp32; zero deltas.  -> (logits, deltas, anchors)."""
    g = torch.Generator().manual_seed(seed)
    anchors = anchors_for(S_SHAPES, (A, A), 4, g, device)
    counts = [h * w * A for h, w in S_SHAPES]
    n = sum(counts)
    rows = []
    for _ in range(images):
        p = torch.linspace(0.002, 0.11, n * C, dtype=torch.float64)[torch.randperm(n * C, generator=g)].reshape(n, C)
        p = torch.cat([p, 1 - p.sum(1, keepdim=True)], 1)
        assert float(p[:, -1].min()) >= 0.12 - 1e-12
        shift = (torch.rand((n, 1), generator=g, dtype=torch.float64) * 2 - 1) * 60
        rows.append((p.log() + shift).float())
    flat = torch.stack(rows)   # (B, n, K), anchors in level order, ((h W + w) A + a) inside a level
    cls, box, lo = [], [], 0
    for (h, w), cnt in zip(S_SHAPES, counts):
        lv = flat[:, lo:lo + cnt].contiguous()
        if layout == 'nchw':
            lv = lv.reshape(images, h, w, A * (C + 1)).permute(0, 3, 1, 2).contiguous()
            box.append(torch.zeros((images, A * 4, h, w), device=device))
        else:
            box.append(torch.zeros((images, cnt, 4), device=device))
        cls.append(lv.to(device))
        lo += cnt
    return cls, box, anchors


def f64_selection(logits_level, K, score_thr, nms_pre):
    """One image's level (A K, H, W) or (n, K) -> (flat candidate indices anchor C + c of the first min(nms_pre, #valid) in
    (f64 probability descending, index ascending) order, their f64 probabilities, #valid)."""
    t = logits_level.cpu()
    p = f64_probs(t[None], K)[0]
    flat = (p.permute(1, 2, 0) if p.dim() == 3 else p).reshape(-1)
    valid = torch.nonzero(flat > score_thr).squeeze(1)
    order = valid[torch.sort(flat[valid], descending=True, stable=True).indices]
    return order[:nms_pre], flat[order[:nms_pre]], int(valid.numel())
