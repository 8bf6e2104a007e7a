"""GPU: float16 / bfloat16 head outputs read in place by the five multi-level entries (`sph2pob_*_h16`).

The contract (include/sph2pob_hip.h): a level value is widened on load and everything after is the fp32
entry's arithmetic, so for levels from the allocator
  * the loss has the BITS of the fp32 entry on `x.float()`;
  * the gradient is RNE_T(s * g) — s the fp32 entry's stash value, g the upstream gradient, one fp32 product and one narrowing —
    which is the fp32 call's gradient narrowed with `.to(dtype)`, bit for bit (NaNs compared as NaNs);
  * the four inference outputs are bit-equal to the call on `.float()` copies.
Shapes are the smallest at which each addressing path can go wrong: the vector kind (H W a multiple of 4), the scalar kind, a
flattened level; for the regression losses a full and a partial span, a span with no live row, both weight shapes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
UPSTREAM = (1.0, 0.5, 3.0, 65536.0)   # 1: every workgroup of the first backward returns at once; the others recompute
B, C, A_REG = 2, 3, 9


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


def same_bits(a, b):
    """Bit equality of two 16-bit tensors, NaNs compared as NaNs."""
    assert a.dtype is b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(torch.int16) != b.view(torch.int16)))
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        print(f'{int(bad.sum())} of {bad.numel()} differ; first:',
              [(i, hex(int(a[tuple(i)].view(torch.int16)) & 0xffff), hex(int(b[tuple(i)].view(torch.int16)) & 0xffff)) for i in idx])
        return False
    return True


def check_loss_and_gradients(fn, levels, dtype):
    """fn(levels) -> loss.  Loss bits, gradient dtype, and the gradient for every upstream gradient — first backward and a second
    one through the retained graph — against the fp32 call narrowed once."""
    xs = [x.clone().requires_grad_(True) for x in levels]
    fs = [x.float().requires_grad_(True) for x in levels]
    with torch.no_grad():
        assert torch.equal(fn(xs), fn(fs))   # the forward-only instantiation too
    for g in UPSTREAM:
        loss, ref = fn(xs), fn(fs)
        assert loss.dtype is torch.float32 and torch.isfinite(loss) and float(loss) != 0.0
        assert torch.equal(loss.view(torch.int32), ref.view(torch.int32)), (float(loss), float(ref))
        want = [w.to(dtype) for w in torch.autograd.grad(ref * g, fs)]
        first = torch.autograd.grad(loss * g, xs, retain_graph=True)
        kept = [v.clone() for v in first]
        again = torch.autograd.grad(loss * g, xs)
        for l, (a, b, w) in enumerate(zip(kept, again, want)):
            assert a.dtype is dtype and b.dtype is dtype
            assert bool((w != 0).any()), (g, l)
            assert same_bits(a, w), (g, l, 'first backward')
            assert same_bits(b, w), (g, l, 'second backward')
    return want


# ---- focal ----

def focal_scene(dtype):
    g = torch.Generator().manual_seed(11)
    shapes = [(B, 2 * C, 4, 8), (B, 2 * C, 3, 5), (B, 7, C)]   # vector kind, scalar kind, flattened
    levels = []
    for s in shapes:
        x = torch.rand(s, generator=g) * 24 - 12
        flat = x.view(-1)
        flat[torch.randperm(flat.numel(), generator=g)[:4]] = torch.tensor([30.0, -30.0, 30.0, -30.0])
        levels.append(x.to(dtype).cuda())
    n = 2 * 32 + 2 * 15 + 7
    labels = (torch.arange(B * n) % (C + 1)).view(B, n)[:, torch.randperm(n, generator=g)].contiguous()   # every class and the background
    weights = torch.tensor([0.0, 1.0, 0.5, 2.0])[torch.randint(0, 4, (B, n), generator=g)]
    assert bool((weights == 0).any()) and set(labels.unique().tolist()) == set(range(C + 1))
    return levels, labels.cuda(), weights.cuda()


@pytest.mark.parametrize('dtype', DTYPES)
def test_focal_loss_bits_and_gradients(S, dtype):
    levels, labels, weights = focal_scene(dtype)
    avg = torch.tensor([7.0], device='cuda')
    want = check_loss_and_gradients(lambda xs: S.sph_focal_loss(xs, labels, weights, avg_factor=avg), levels, dtype)
    if dtype is torch.float16:   # the inputs reach the subnormal range of fp16: those gradients are kept, not flushed
        tiny = torch.finfo(torch.float16).smallest_normal
        assert any(bool(((w.float().abs() > 0) & (w.float().abs() < tiny)).any()) for w in want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_focal_element_weights_and_host_divisor(S, dtype):
    levels, labels, weights = focal_scene(dtype)
    w3 = (weights[:, :, None] * torch.tensor([1.0, 0.25, 2.0], device='cuda')).contiguous()
    check_loss_and_gradients(lambda xs: S.sph_focal_loss(xs, labels, w3, avg_factor=5.0, gamma=1.5, alpha=0.4), levels, dtype)


# ---- regression losses ----

def box_scene(dtype, dim, per_component):
    """Levels (a full + a partial span, vector store; scalar store; flattened), anchors, decoded and encoded targets, weights with
    about a tenth of the rows live, image 1's whole second level dead, and a NaN among a dead row's deltas."""
    g = torch.Generator().manual_seed(12 + dim)
    shapes = [(B, A_REG * dim, 5, 8), (B, A_REG * dim, 3, 5), (B, 11, dim)]
    ns = [A_REG * 40, A_REG * 15, 11]
    n = sum(ns)
    levels = [(torch.randn(s, generator=g) * 0.1) for s in shapes]
    live = torch.rand((B, n), generator=g) < 0.1
    live[1, ns[0]:ns[0] + ns[1]] = False   # spans with no live row
    live[0, 0] = live[0, ns[0] + 1] = live[1, n - 1] = True
    live[0, 5] = False
    levels[0][0, 0 * dim + 1, 0, 5] = float('nan')   # anchor 5 * A + 0 of image 0 ...
    live[0, 5 * A_REG] = False                       # ... is dead
    u = torch.rand((n, 5), generator=g)
    anchors = torch.stack([u[:, 0] * 360, 30 + u[:, 1] * 120, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50, u[:, 4] * 120 - 60], 1)[:, :dim].contiguous()
    boxes = anchors[None] + torch.randn((B, n, dim), generator=g) * torch.tensor([2.0, 2.0, 1.0, 1.0, 3.0])[:dim]
    deltas = torch.randn((B, n, dim), generator=g) * 0.1
    weights = live.float() * (0.5 + torch.rand((B, n), generator=g))
    if per_component:
        weights = (weights[:, :, None] * torch.tensor([1.0, 1.0, 0.5, 2.0, 1.0])[:dim]).contiguous()
    return [x.to(dtype).cuda() for x in levels], anchors.cuda(), boxes.contiguous().cuda(), deltas.cuda(), weights.cuda()


def check_dead_nan_is_inert(grads, dim):
    assert float(grads[0][0, 1, 0, 5]) == 0.0 and not bool(torch.isnan(grads[0][0, :dim, 0, 5]).any())


@pytest.mark.parametrize('per_component', (False, True))
@pytest.mark.parametrize('dim', (4, 5))
@pytest.mark.parametrize('dtype', DTYPES)
def test_delta_loss_bits_and_gradients(S, dtype, dim, per_component):
    levels, _, _, deltas, weights = box_scene(dtype, dim, per_component)
    avg = torch.tensor([9.0], device='cuda')
    beta = 0.05 if per_component else 0.0   # SmoothL1 and L1
    want = check_loss_and_gradients(lambda xs: S.sph_delta_loss(xs, deltas, weights, beta=beta, avg_factor=avg), levels, dtype)
    check_dead_nan_is_inert(want, dim)


@pytest.mark.parametrize('per_component', (False, True))
@pytest.mark.parametrize('dim', (4, 5))
@pytest.mark.parametrize('dtype', DTYPES)
def test_bbox_loss_bits_and_gradients(S, dtype, dim, per_component):
    levels, anchors, boxes, _, weights = box_scene(dtype, dim, per_component)
    coder = (S.DeltaXYWHSphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2)) if dim == 4
             else S.DeltaXYWHASphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)))
    avg = torch.tensor([9.0], device='cuda')
    want = check_loss_and_gradients(lambda xs: S.sph_bbox_loss(xs, anchors, boxes, weights, bbox_coder=coder, mode='ciou', avg_factor=avg),
                                    levels, dtype)
    check_dead_nan_is_inert(want, dim)


# ---- capture ----

def test_focal_forward_backward_capture_on_bf16_levels(S):
    """sph_focal_loss -> backward on bf16 levels captured first, then replayed twice with changed logits against the eager step:
    one stream, nothing read back, the device-side skip test inside the graph."""
    levels, labels, weights = focal_scene(torch.bfloat16)
    avg = torch.tensor([7.0], device='cuda')
    ins = [x.clone().requires_grad_(True) for x in levels]

    def step():
        loss = S.sph_focal_loss(ins, labels, weights, avg_factor=avg)
        return (loss,) + torch.autograd.grad(loss * 0.5, ins)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (21, 22):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for x in ins:
                x.copy_((torch.rand(x.shape, generator=g) * 16 - 8).to(torch.bfloat16))
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.isfinite(got[0]) and float(got[0]) > 0
        for a, b in zip(got[1:], want[1:]):
            assert a.dtype is torch.bfloat16 and same_bits(a, b) and bool((a != 0).any())


# ---- memory ----

def test_focal_memory_no_fp32_copy_and_no_fp32_stash(S):
    """One bf16 NCHW level of N elements: forward + backward holds the 2 N stash that becomes the gradient (and 2 N more when
    autograd clones it) — never the 4 N fp32 copy and the 4 N fp32 stash; forward only holds neither."""
    shape = (2, 72, 64, 64)
    N = 2 * 72 * 64 * 64
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(shape, generator=g) * 3).to(torch.bfloat16).cuda().requires_grad_(True)
    n = 9 * 64 * 64
    labels = torch.randint(0, 9, (2, n), generator=g).cuda()
    avg = torch.tensor([50.0], device='cuda')

    def train():
        S.sph_focal_loss([x], labels, None, avg_factor=avg).backward()

    def infer():
        with torch.no_grad():
            return S.sph_focal_loss([x], labels, None, avg_factor=avg)

    figures = {}
    for name, fn in (('forward + backward', train), ('forward only', infer)):
        fn()   # warm-up: the workspace of this shape is cached from here on
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        figures[name] = torch.cuda.max_memory_allocated() - before
        print(f'h16 focal memory, {name}: peak {figures[name]} bytes = {figures[name] / N:.2f} N')
        assert x.grad is None if fn is infer else x.grad.dtype is torch.bfloat16
    assert figures['forward + backward'] <= 5 * N, figures
    assert figures['forward only'] <= N, figures


# ---- inference ----

def detection_scene(dtype):
    g = torch.Generator().manual_seed(31)
    hw = [(4, 8), (3, 5)]
    cls = [(torch.rand((B, 2 * C, h, w), generator=g) ** 4).to(dtype).cuda() for h, w in hw]   # already rounded: both calls see these values
    box = [(torch.randn((B, 2 * 4, h, w), generator=g) * 0.5).to(dtype).cuda() for h, w in hw]
    anchors = []
    for h, w in hw:
        u = torch.rand((2 * h * w, 4), generator=g)
        anchors.append(torch.stack([u[:, 0] * 360, 30 + u[:, 1] * 120, 10 + u[:, 2] * 40, 10 + u[:, 3] * 40], 1).cuda())
    return cls, box, anchors


def same_detections(a, b):
    assert int(a.num_dets.sum()) > 0
    for name in ('dets', 'labels', 'prior_inds', 'num_dets'):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype is y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name


@pytest.mark.parametrize('dtype', DTYPES)
def test_get_bboxes_equals_the_call_on_fp32_copies(S, dtype):
    cls, box, anchors = detection_scene(dtype)
    kw = dict(bbox_coder=S.DeltaXYWHSphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2)), score_thr=0.05, nms_pre=16,
              nms=dict(type='nms', iou_threshold=0.5), max_per_img=8, activation='none')
    same_detections(S.sph_get_bboxes(cls, box, anchors, **kw), S.sph_get_bboxes([c.float() for c in cls], [d.float() for d in box], anchors, **kw))


@pytest.mark.parametrize('calculator', ('unbiased_iou', 'planar'))
@pytest.mark.parametrize('dtype', DTYPES)
def test_test_bboxes_equals_the_call_on_fp32_copies(S, dtype, calculator):
    cls, box, anchors = detection_scene(dtype)
    cfg = dict(nms_pre=16, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=8,
               iou_calculator=calculator, box_formator='sph2pix')
    kw = dict(bbox_coder=S.DeltaXYWHSphBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2)), test_cfg=cfg, activation='none')
    same_detections(S.sph_test_bboxes(cls, box, anchors, **kw), S.sph_test_bboxes([c.float() for c in cls], [d.float() for d in box], anchors, **kw))
    logits = [torch.logit(c.float().clamp(1e-4, 1 - 1e-4)).to(dtype) for c in cls]   # and through the sigmoid
    kw['activation'] = 'sigmoid'
    same_detections(S.sph_test_bboxes(logits, box, anchors, **kw), S.sph_test_bboxes([c.float() for c in logits], [d.float() for d in box], anchors, **kw))
