"""GPU box: time BASELINE.json configs[2] (Sph2Pob + CIoU loss fwd+bwd, 1M RBFoV) and configs[3] (MaxIoUAssigner
overlaps 64 GT x ~98k anchors + SphNMS on 5000 boxes / 37 classes) on one MI355X.  One JSON line per config."""
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sph_retina_amd as S  # noqa: E402
from sph_retina_amd.losses import Sph2PobIoULoss  # noqa: E402
from sph_retina_amd.bbox.nms import SphNMS  # noqa: E402


def timeit(fn, warm=5, reps=30, settle_s=0.03):
    """Seconds per call, HIP events around `reps` back-to-back calls.  After `warm` calls the function is repeated for
    another `settle_s` seconds untimed: the clocks drop while the host prepares inputs and only recover after a few
    thousand launches (a 14 us kernel measured right after an idle gap reads 32 us)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_s:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def pmc_roofline(kernel_prefix, seconds, algorithmic_bytes, grid=None, gauss=False):
    """What bounds a kernel, from this round's committed counter passes (profiles/configs_pmc_summary.json, made by
    tools/profile_configs_pmc.sh + tools/summarize_configs_pmc.py): HBM-side bytes per launch (FETCH_SIZE x 2 + WRITE_SIZE, the
    guide's gfx950 correction) and the VALU issue-slot fraction, next to the algorithmic bytes and THIS run's time.
    The IoU and Gaussian losses share their kernel templates: `gauss` picks the kernels with the GaussBody template argument,
    otherwise those are left out."""
    out = {'algorithmic_bytes': algorithmic_bytes, 'hbm_frac_algorithmic': algorithmic_bytes / seconds / 8e12 if algorithmic_bytes else None}
    try:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'configs_pmc_summary.json')) as f:
            ks = json.load(f)['kernels']
    except (OSError, ValueError):
        return out
    cands = [e for k, e in ks.items() if e['kernel'].startswith(kernel_prefix) and ('GaussBody' in e['kernel']) == gauss and
             (grid is None or e['grid_threads'] == grid)]
    if not cands:
        return out
    e = max(cands, key=lambda c: c['grid_threads'])
    out.update(kernel=e['kernel'], counter_bytes=e.get('hbm_bytes'), fetch_calibrated=e.get('fetch_calibrated'),
               hbm_frac_counter_bytes=(e['hbm_bytes'] / seconds / 8e12) if e.get('hbm_bytes') else None,
               valu_issue_frac=e.get('valu_issue_frac'), valu_insts_per_wave=e.get('valu_insts_per_wave'), binds=e.get('binds'),
               profiled_kernel_us=e['avg_ns'] / 1e3, source='profiles/configs_pmc_summary.json')
    return out


def boxes(n, seed, dim=4, alpha=(1, 100), gamma=(-90, 90)):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((n, 5), generator=g)
    cols = [u[:, 0] * 360, u[:, 1] * 180, u[:, 2] * (alpha[1] - alpha[0]) + alpha[0],
            u[:, 3] * (alpha[1] - alpha[0]) + alpha[0]]
    if dim == 5:
        cols.append(u[:, 4] * (gamma[1] - gamma[0]) + gamma[0])
    return torch.stack(cols, 1).cuda()


def config3(n=1_000_000):
    tgt = boxes(n, 0, 5, alpha=(5, 90), gamma=(-60, 60))
    g = torch.Generator().manual_seed(1)
    pred = tgt + (torch.randn((n, 5), generator=g) * torch.tensor([8., 8., 6., 6., 10.])).cuda()
    pred[:, 0] %= 360
    pred[:, 1].clamp_(1, 179)
    pred[:, 2:4].clamp_(1, 170)
    pred.requires_grad_(True)
    loss = Sph2PobIoULoss(mode='ciou', reduction='mean')

    def step():
        pred.grad = None
        loss(pred, tgt).backward()
    t = timeit(step)
    tf = timeit(lambda: loss(pred.detach(), tgt))
    # the same work through the C ABI directly (no autograd / Python object overhead): fwd kernel + 2-pass sum + bwd kernel
    import ctypes
    from sph_retina_amd import _lib, _torch_glue as G
    lib = _lib.lib()
    p_, t_ = pred.detach().contiguous(), tgt.contiguous()
    elem, out = torch.empty(n, device='cuda'), torch.empty((), device='cuda')
    ws = torch.empty(lib.sph2pob_sum_workspace_floats(), device='cuda')
    gp, one = torch.empty_like(p_), torch.ones((), device='cuda')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nn, null = ctypes.c_int64(n), ctypes.c_void_p(0)

    ws2 = torch.empty(lib.sph2pob_loss_sum_workspace_floats(n), device='cuda')

    stash = torch.empty_like(p_)

    def abi_step():   # what the autograd Function launches: forward + gradients in one pass, final sum, backward = scale
        lib.sph2pob_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null, ctypes.c_void_p(out.data_ptr()),
                                      G.ptr(ws2), G.ptr(stash), null, nn, 5, 3, ctypes.c_float(1e-6), st)
        lib.sph2pob_loss_grad_scale_f32(G.ptr(stash), ctypes.c_void_p(one.data_ptr()), 0, G.ptr(stash), nn, 5, st)   # in place, g = 1

    def abi_step_two_pass():   # round 1's form: forward (+ sum), then a backward kernel that recomputes the forward
        lib.sph2pob_loss_fwd_sum_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), ctypes.c_void_p(out.data_ptr()),
                                     G.ptr(ws2), nn, 5, 3, ctypes.c_float(1e-6), st)
        lib.sph2pob_loss_bwd_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_void_p(one.data_ptr()), 0, ctypes.c_float(1.0 / n),
                                 G.ptr(gp), null, nn, 5, 3, ctypes.c_float(1e-6), st)
    half = torch.full((), 0.5, device='cuda')

    def abi_step_scaled():   # an upstream gradient other than 1 (loss_weight, a loss summed with others and rescaled): the 40 MB scale pass runs
        lib.sph2pob_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null, ctypes.c_void_p(out.data_ptr()),
                                      G.ptr(ws2), G.ptr(stash), null, nn, 5, 3, ctypes.c_float(1e-6), st)
        lib.sph2pob_loss_grad_scale_f32(G.ptr(stash), ctypes.c_void_p(half.data_ptr()), 0, G.ptr(gp), nn, 5, st)
    def abi_step_root():   # the loss is the root of the graph (upstream gradient 1 known on the host: a C / C++ training loop):
        # forward + gradients + final sum, no scale launch; and the same without the scalar loss (gradients only)
        lib.sph2pob_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null, ctypes.c_void_p(out.data_ptr()),
                                      G.ptr(ws2), G.ptr(stash), null, nn, 5, 3, ctypes.c_float(1e-6), st)

    def abi_step_grad_only():
        lib.sph2pob_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null, null, null, G.ptr(stash), null, nn, 5, 3,
                                      ctypes.c_float(1e-6), st)
    tb = timeit(abi_step_two_pass)
    ta = timeit(abi_step)
    tr = timeit(abi_step_root)
    tgo = timeit(abi_step_grad_only)
    ts = timeit(abi_step_scaled)
    # the same Python step with the host out of the way: captured once (torch's whole-network recipe: forward, backward
    # and the accumulation into pred.grad in one hipGraph), replayed
    tg = None
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        pred.grad = None
        whole = torch.cuda.CUDAGraph()
        with torch.cuda.graph(whole):
            loss(pred, tgt).backward()
        tg = timeit(whole.replay)
    except Exception as e:   # noqa: BLE001  (reported, not fatal: the table's other figures do not depend on it)
        print('graph capture of the loss step failed:', e, file=sys.stderr)
    return {'config': 'configs[2]: 1,000,000 RBFoV pairs, Sph2Pob + CIoU loss forward+backward', 'pairs': n,
            'autograd_fwd_bwd_ms': t * 1e3, 'autograd_fwd_ms': tf * 1e3, 'c_abi_fwd_bwd_ms': ta * 1e3, 'c_abi_root_loss_ms': tr * 1e3, 'c_abi_gradients_only_ms': tgo * 1e3,
            'c_abi_two_pass_fwd_bwd_ms': tb * 1e3, 'c_abi_fwd_bwd_scaled_grad_ms': ts * 1e3, 'graph_replay_fwd_bwd_ms': tg * 1e3 if tg else None,
            'pairs_per_s_c_abi': n / ta, 'pairs_per_s_autograd': n / t, 'pairs_per_s_graph_replay': n / tg if tg else None,
            'algorithmic_bytes_per_pair': 108, 'hbm_GBps_c_abi': 108 * n / ta / 1e9,
            'roofline': pmc_roofline('loss_fwd_grad_kernel', ta, 60.0 * n),
            'hbm_frac_of_8TBps_c_abi': 108 * n / ta / 8e12,
            'note': 'c_abi = loss_fwd_grad (forward + gradients + per-workgroup partial sums in one pass) + final sum + '
                    'grad_scale through the C ABI; two_pass = loss_fwd_sum + final sum + loss_bwd (recomputes the forward); '
                    'autograd = the c_abi launches behind torch.autograd (one Function node), host-bound; graph_replay = that Python '
                    'step (incl. the accumulation into pred.grad) captured once into a hipGraph and replayed'}


def retina_anchors(h=512, w=1024):
    """5-level, 9-anchor RetinaNet grid (strides 8..128, octave_base_scale 4, 3 scales x 3 ratios) mapped pixel->sph
    as sphdet/bbox/box_formator.py:85-92: (x/W*360, y/H*180, w/W*360, h/H*180)."""
    out = []
    for stride in (8, 16, 32, 64, 128):
        fh, fw = math.ceil(h / stride), math.ceil(w / stride)
        ys, xs = torch.meshgrid(torch.arange(fh) * stride, torch.arange(fw) * stride, indexing='ij')
        for sc in (2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3)):
            for ratio in (0.5, 1.0, 2.0):
                size = 4 * stride * sc
                ww, hh = size / math.sqrt(ratio), size * math.sqrt(ratio)
                out.append(torch.stack([xs.flatten() / w * 360, ys.flatten() / h * 180,
                                        torch.full((fh * fw,), ww / w * 360), torch.full((fh * fw,), hh / h * 180)], 1))
    a = torch.cat(out).float()
    a[:, 1].clamp_(0.5, 179.5)
    return a.cuda()


def config4(h=512, w=1024):
    anchors = retina_anchors(h, w)
    g = torch.Generator().manual_seed(0)
    u = torch.rand((64, 4), generator=g)
    gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda()
    calc = S.SphOverlaps2D(backend='sph2pob_standard_iou', box_version=4)
    t_iou = timeit(lambda: calc(gt, anchors))
    ov = calc(gt, anchors)

    def assign():
        o = calc(gt, anchors)
        mx, am = o.max(dim=0)
        gmx, gam = o.max(dim=1)
        return mx, am, gmx, gam
    t_assign = timeit(assign)
    from sph_retina_amd.bbox.assigners import SphMaxIoUAssigner
    fused = SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1)
    labels = torch.randint(0, 37, (64,)).cuda()
    t_fused = timeit(lambda: fused.assign(anchors, gt, gt_labels=labels))
    matrix = SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1, fused=False)
    t_matrix = timeit(lambda: matrix.assign(anchors, gt, gt_labels=labels))
    # the same two routes through the C ABI with every buffer allocated once (what a captured graph or a C++ caller pays)
    from sph_retina_amd import _lib, _torch_glue as G
    lib = _lib.lib()
    kk, nn = gt.size(0), anchors.size(0)
    st = G.raw_stream_of(gt.device)
    mo, gi, lab = torch.empty(nn, device='cuda'), torch.empty(nn, dtype=torch.int64, device='cuda'), torch.empty(nn, dtype=torch.int64, device='cuda')
    amo, gm, gam = torch.empty(nn, dtype=torch.int64, device='cuda'), torch.empty(kk, device='cuda'), torch.empty(kk, dtype=torch.int64, device='cuda')
    wsf = torch.empty(lib.sph2pob_iou_assign_workspace_bytes(kk, nn) // 8, dtype=torch.int64, device='cuda')
    stf = torch.zeros(lib.sph2pob_iou_assign_state_bytes(kk, nn) // 8, dtype=torch.int64, device='cuda')
    wsm = torch.empty(lib.sph2pob_assign_workspace_bytes(kk, nn) // 8, dtype=torch.int64, device='cuda')
    ovb = torch.empty((kk, nn), device='cuda')

    def fused_abi():
        lib.sph2pob_iou_assign_f32(G.ptr(gt), kk, G.ptr(anchors), nn, 4, 0, 0, None, None, 0.5, 0.0, 0.4, 0.0, 1, 1, G.ptr(labels),
                                   G.ptr(mo), None, None, None, G.ptr(gi), G.ptr(lab), G.ptr(wsf), G.ptr(stf), st)

    def matrix_abi():
        lib.sph2pob_iou_pairwise_f32(G.ptr(gt), kk, G.ptr(anchors), nn, G.ptr(ovb), 4, 0, 0, 0, 0, st)
        lib.sph2pob_assign_f32(G.ptr(ovb), kk, nn, 0.5, 0.0, 0.4, 0.0, 1, 1, G.ptr(labels), G.ptr(mo), G.ptr(amo), G.ptr(gm),
                               G.ptr(gam), G.ptr(gi), G.ptr(lab), G.ptr(wsm), st)
    t_fused_abi, t_matrix_abi = timeit(fused_abi, reps=200), timeit(matrix_abi, reps=200)
    k = 5000
    rng = np.random.default_rng(4)
    centres = boxes(300, 8, alpha=(5, 60)).cpu().numpy()
    b = centres[rng.integers(0, 300, k)] + rng.standard_normal((k, 4)).astype(np.float32) * 2.0
    b[:, 0] %= 360
    b[:, 1] = b[:, 1].clip(1, 179)
    b[:, 2:] = b[:, 2:].clip(2, 120)
    nb, ns, ni = torch.from_numpy(b).cuda(), torch.rand(k).cuda(), torch.randint(0, 37, (k,)).cuda()
    nms = SphNMS('sph2pob_efficient')
    cfg = dict(type='nms', iou_threshold=0.5, max_num=100)
    t_nms = timeit(lambda: nms(nb, ns, ni, cfg), reps=20)
    t_nms1 = timeit(lambda: nms(nb, ns, torch.zeros_like(ni), cfg), reps=10)
    # the launcher alone (buffers allocated once, no host read of the count): what a captured graph or a C++ caller pays
    wsn = torch.empty(lib.sph2pob_batched_nms_workspace_bytes(k, 4), dtype=torch.uint8, device='cuda')
    kout, dout, stat = torch.empty(100, dtype=torch.int64, device='cuda'), torch.empty((100, 5), device='cuda'), torch.empty(1, dtype=torch.int32, device='cuda')
    ni64 = ni.to(torch.int64)
    t_nms_abi = timeit(lambda: lib.sph2pob_batched_nms_f32(G.ptr(nb), G.ptr(ns), G.ptr(ni64), k, 4, 1, 0.5, 100, G.ptr(wsn), G.ptr(kout),
                                                            G.ptr(dout), G.ptr(stat), st), reps=100)
    kall, dall = torch.empty(k, dtype=torch.int64, device='cuda'), torch.empty((k, 5), device='cuda')
    t_nms1_abi = timeit(lambda: lib.sph2pob_batched_nms_f32(G.ptr(nb), G.ptr(ns), None, k, 4, 1, 0.5, k, G.ptr(wsn), G.ptr(kall),
                                                             G.ptr(dall), G.ptr(stat), st), reps=50)
    m, n = ov.shape
    roof = {'pairwise': pmc_roofline('iou_pairwise_compact_kernel<0, 4, true, 1>', t_iou, 16.0 * (m + n) + 4.0 * m * n, grid=((n + 255) // 256) * 256 * (8 if n < 200000 else 3)),
            'fused_phase1': pmc_roofline('iou_pairwise_compact_kernel<0, 4, true, 2>', t_fused_abi, 16.0 * (m + n), grid=((n + 255) // 256) * 256 * (8 if n < 200000 else 3)),
            'nms_mask': pmc_roofline('nms_mask_compact_kernel', t_nms_abi, None), 'nms_sweep': pmc_roofline('nms_sweep_kernel', t_nms_abi, None)}
    return {'config': 'configs[3]: MaxIoUAssigner overlaps 64 GT x %d anchors (%dx%d ERP grid) + SphNMS 5000 boxes' % (n, h, w),
            'pairs': m * n, 'iou_matrix_ms': t_iou * 1e3, 'pairs_per_s': m * n / t_iou,
            'iou_plus_torch_max_argmax_ms': t_assign * 1e3, 'fused_assign_total_ms': t_fused * 1e3, 'matrix_assign_total_ms': t_matrix * 1e3,
            'fused_assign_c_abi_ms': t_fused_abi * 1e3, 'matrix_assign_c_abi_ms': t_matrix_abi * 1e3, 'frac_pairs_overlapping': float((ov > 0).float().mean()),
            'nms_5000x37cls_ms': t_nms * 1e3, 'nms_5000_single_class_ms': t_nms1 * 1e3,
            'nms_5000x37cls_c_abi_ms': t_nms_abi * 1e3, 'nms_5000_single_class_c_abi_ms': t_nms1_abi * 1e3, 'roofline': roof}


def config4_batch(images=8, num_gt=64, h=512, w=1024, rounds=7):
    """Anchor targets for a minibatch (sph2pob_anchor_targets_f32) against the per-image loop it replaces, through the C ABI
    with every buffer allocated once: (a) the batched entry, two launches for all images; (b) `images` calls of
    sph2pob_iou_assign_f32 on the same data; (c) = (b) + the torch target construction of tools/demo_hot_path.py's
    single-image step per image (boolean-mask indexing and int(pos.sum()): host synchronisations).  The three are timed in
    alternation `rounds` times in this one process; the spread of (b) over the rounds is the yardstick for (a) <= (b)."""
    from sph_retina_amd import _lib, _torch_glue as G
    lib = _lib.lib()
    anchors = retina_anchors(h, w)
    n, K = anchors.size(0), images * num_gt
    g = torch.Generator().manual_seed(0)
    u = torch.rand((K, 4), generator=g)
    gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda()
    labels = torch.randint(0, 37, (K,), generator=g).cuda()
    off = (torch.arange(images + 1) * num_gt).cuda()
    st = G.raw_stream_of(gt.device)
    i64, f32 = dict(dtype=torch.int64, device='cuda'), dict(dtype=torch.float32, device='cuda')
    o = [torch.empty((images, n), **i64), torch.empty((images, n), **f32), torch.empty((images, n), **i64), torch.empty((images, n), **i64),
         torch.empty((images, n), **f32), torch.empty((images, n, 4), **f32), torch.empty((images, n, 4), **f32), torch.empty(images, **i64),
         torch.empty(images, **i64), torch.empty(1, **f32)]
    op = [G.ptr(t) for t in o]
    wsb = torch.empty(lib.sph2pob_anchor_targets_workspace_bytes(images, K, num_gt, n) // 8, **i64)
    stb = torch.zeros(lib.sph2pob_anchor_targets_state_bytes(images, num_gt, n) // 8, **i64)
    ws1 = torch.empty(lib.sph2pob_iou_assign_workspace_bytes(num_gt, n) // 8, **i64)
    st1 = torch.zeros(lib.sph2pob_iou_assign_state_bytes(num_gt, n) // 8, **i64)
    mo, gi, lab = torch.empty((images, n), **f32), torch.empty((images, n), **i64), torch.empty((images, n), **i64)
    import ctypes
    cf = [ctypes.c_float(v) for v in (0.5, 0.0, 0.4, 0.0, -1.0)]

    def batched():
        rc = lib.sph2pob_anchor_targets_f32(G.ptr(anchors), n, G.ptr(gt), G.ptr(labels), G.ptr(off), images, K, num_gt, 4, 0, 0, cf[0], cf[1],
                                            cf[2], cf[3], 1, 1, 37, cf[4], 0, None, None, *op, G.ptr(wsb), G.ptr(stb), st)
        assert rc == 0, rc

    def loop():
        for b in range(images):
            lib.sph2pob_iou_assign_f32(G.ptr(gt[b * num_gt:]), num_gt, G.ptr(anchors), n, 4, 0, 0, None, None, 0.5, 0.0, 0.4, 0.0, 1, 1,
                                       G.ptr(labels[b * num_gt:]), G.ptr(mo[b]), None, None, None, G.ptr(gi[b]), G.ptr(lab[b]), G.ptr(ws1),
                                       G.ptr(st1), st)

    def loop_targets():
        loop()
        total = 0
        for b in range(images):
            pos = gi[b] > 0
            total += max(int(pos.sum()), 1)
            bbox_targets = torch.zeros_like(anchors)
            bbox_weights = torch.zeros_like(anchors)
            bbox_targets[pos] = gt[b * num_gt:(b + 1) * num_gt][gi[b][pos] - 1]
            bbox_weights[pos] = 1.0
        return total
    batched(), loop()
    torch.cuda.synchronize()
    assert torch.equal(o[0], gi) and torch.equal(o[1], mo) and torch.equal(o[2], lab), 'batched and per-image assignments differ'
    assert float(o[9]) == float(loop_targets())
    ta, tb, tc = [], [], []
    for _ in range(rounds):
        ta.append(timeit(batched, reps=200) * 1e6)
        tb.append(timeit(loop, reps=200) * 1e6)
        tc.append(timeit(loop_targets, reps=20) * 1e6)
    med = lambda v: float(np.median(v))
    return {'config': 'anchor targets: %d images x %d GT x %d anchors (%dx%d ERP grid), C ABI' % (images, num_gt, n, h, w),
            'a_batched_us': med(ta), 'b_loop_assign_us': med(tb), 'c_loop_assign_plus_torch_targets_us': med(tc),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'b_spread_us': max(tb) - min(tb),
            'a_over_b': med(ta) / med(tb), 'a_over_c': med(ta) / med(tc), 'num_pos': o[7].tolist(),
            'note': '(a) also writes labels, label_weights, bbox_targets, bbox_weights and the counts, which (b) does not'}


def train_targets(images=8, num_gt=64, h=512, w=1024, rounds=5, backends=None):
    """`sph_train_targets` on the backends without a closed form (sph2pob_anchor_targets_any_f32: two launches for the batch)
    against the per-image API it replaces — `SphMaxIoUAssigner.assign` on each image (the pairwise kernel into a (k, n) matrix,
    then the three launches of the matrix epilogue) plus the torch target lines of `_get_targets_single` with their `nonzero`
    synchronisations — both through the Python API, timed in alternation `rounds` times in this one process.  One JSON record per
    backend; `loop_spread_us` over the rounds is the yardstick for the ratio.  No cull on either side: every pair is evaluated."""
    import sph_retina_amd as S
    anchors = retina_anchors(h, w)
    n, K = anchors.size(0), images * num_gt
    g = torch.Generator().manual_seed(0)
    u = torch.rand((K, 5), generator=g)
    gt5 = torch.stack([u[:, 0] * 300 + 30, 50 + u[:, 1] * 80, 10 + u[:, 2] * 35, 10 + u[:, 3] * 35, -40 + 80 * u[:, 4]], 1).cuda()
    labels = torch.randint(0, 37, (K,), generator=g).cuda()
    anchors5 = torch.cat([anchors, ((torch.arange(n, device='cuda') % 7) - 3.0).unsqueeze(1) * 10], 1).contiguous()
    off = (torch.arange(images + 1) * num_gt).cuda()
    out = []
    for backend, dim in (backends or (('sph2pob_legacy_iou', 4), ('sph_iou', 4), ('fov_iou', 4), ('naive_iou', 4), ('naive_iou', 5),
                                      ('unbiased_iou', 4), ('unbiased_iou', 5))):
        cfg = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                 iou_calculator=dict(type='SphOverlaps2D', backend=backend, box_version=dim)),
                   allowed_border=-1, pos_weight=-1, debug=False)
        a = S.SphMaxIoUAssigner(**{k: v for k, v in cfg['assigner'].items() if k != 'type'})
        bx, gt = (anchors, gt5[:, :4].contiguous()) if dim == 4 else (anchors5, gt5)

        def batched():
            return S.sph_train_targets(bx, gt, labels, off, train_cfg=cfg, num_classes=37, k_max=num_gt)

        def loop():
            total, res = 0, []
            for b in range(images):
                gb, lb = gt[b * num_gt:(b + 1) * num_gt], labels[b * num_gt:(b + 1) * num_gt]
                r = a.assign(bx, gb, gt_labels=lb)
                pos = torch.nonzero(r.gt_inds > 0, as_tuple=False).squeeze(-1)
                neg = torch.nonzero(r.gt_inds == 0, as_tuple=False).squeeze(-1)
                bbox_targets, bbox_weights = torch.zeros_like(bx), torch.zeros_like(bx)
                lab, lw = bx.new_full((n,), 37, dtype=torch.long), bx.new_zeros(n)
                if len(pos) > 0:
                    bbox_targets[pos] = gb[r.gt_inds[pos] - 1]
                    bbox_weights[pos] = 1.0
                    lab[pos] = lb[r.gt_inds[pos] - 1]
                    lw[pos] = 1.0
                if len(neg) > 0:
                    lw[neg] = 1.0
                total += max(len(pos), 1)
                res.append((r.gt_inds, lab, bbox_targets))
            return total, res
        t = batched()
        total, res = loop()
        torch.cuda.synchronize()
        equal = float(t.avg_factor) == float(total) and all(torch.equal(t.gt_inds[b], r[0]) and torch.equal(t.labels[b], r[1]) and
                                                           torch.equal(t.bbox_targets[b], r[2]) for b, r in enumerate(res))
        one = timeit(batched, warm=1, reps=1, settle_s=0.0)
        reps = max(3, min(100, int(0.2 / max(one, 1e-6))))
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timeit(batched, warm=2, reps=reps) * 1e6)
            tb.append(timeit(loop, warm=2, reps=max(3, reps // 4)) * 1e6)
        med = lambda v: float(np.median(v))   # noqa: E731
        out.append({'config': 'train targets: %s dim %d, %d images x %d GT x %d anchors, Python API' % (backend, dim, images, num_gt, n),
                    'batched_us': med(ta), 'loop_us': med(tb), 'batched_rounds_us': ta, 'loop_rounds_us': tb,
                    'batched_spread_us': max(ta) - min(ta), 'loop_spread_us': max(tb) - min(tb), 'batched_over_loop': med(ta) / med(tb),
                    'equal_to_loop': bool(equal), 'num_pos': t.num_pos.tolist()})
        print(json.dumps(out[-1]), flush=True)
    return {'config': 'train targets', 'backends': len(out)}


def get_bboxes(images=8, rounds=7):
    """Detection post-processing for a minibatch (sph_get_bboxes) at the reference's test shape — 512 x 1024 ERP, 5 levels, 9
    anchors, 37 classes, nms_pre 1000, max_per_img 100 — on the head's NCHW outputs: (a) one eager call for the batch; (b) the
    same call replayed from a graph; (c) the per-image composition it replaces (per level: permute, `> thr`, nonzero, stable
    sort, gather, bbox_coder.decode; then sph_batched_nms), looped over the images.  The three are timed in alternation
    `rounds` times in this one process, medians and spreads reported.  `stream_floor_us`: the bytes of one pass over the scores
    over the bandwidth of a device copy of the same tensors measured here (a copy moves each byte twice)."""
    import demo_hot_path as D
    from sph_retina_amd.bbox.nms import sph_batched_nms
    anchors = D.retina_level_anchors()
    cls, box = D.head_outputs(images, 37)
    coder_ = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
    nms = dict(type='nms', iou_threshold=0.5)

    def batched():
        return S.sph_get_bboxes(cls, box, anchors, bbox_coder=coder_, score_thr=0.05, nms_pre=1000, nms=nms, max_per_img=100,
                                iou_calculator='sph2pob_efficient', box_version=4, activation='none')

    def per_image():
        out = []
        for b in range(images):
            bs, ss, ls = [], [], []
            for c, d, a in zip(cls, box, anchors):
                flat = c[b].permute(1, 2, 0).reshape(-1)
                valid = torch.nonzero(flat > 0.05, as_tuple=False).squeeze(1)
                idx = valid[torch.sort(flat[valid], descending=True, stable=True).indices[:1000]]
                ai = torch.div(idx, 37, rounding_mode='floor')
                bs.append(coder_.decode(a[ai], d[b].permute(1, 2, 0).reshape(-1, 4)[ai]))
                ss.append(flat[idx])
                ls.append(idx - ai * 37)
            dets, keep = sph_batched_nms(torch.cat(bs), torch.cat(ss), torch.cat(ls), dict(nms), 'efficient')
            out.append((dets[:100], torch.cat(ls)[keep][:100]))
        return out
    r, ref = batched(), per_image()
    torch.cuda.synchronize()
    for b, ((dets, labels), (d2, l2)) in enumerate(zip(r.to_list(), ref)):
        assert torch.equal(dets, d2) and torch.equal(labels, l2), 'batched and per-image detections differ'
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batched()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batched()
    dst = [torch.empty_like(c) for c in cls]

    def copy():
        for x, y in zip(dst, cls):
            x.copy_(y)
    ta, tb, tc, tcopy = [], [], [], []
    for _ in range(rounds):
        ta.append(timeit(batched, reps=50) * 1e6)
        tb.append(timeit(graph.replay, reps=50) * 1e6)
        tc.append(timeit(per_image, warm=2, reps=5) * 1e6)
        tcopy.append(timeit(copy, reps=50) * 1e6)
    med = lambda v: float(np.median(v))
    score_bytes = sum(c.numel() for c in cls) * 4
    bw = 2 * score_bytes / (med(tcopy) * 1e-6)
    # the kernels' own times in this process: torch's device-activity trace of 20 eager calls, averaged per kernel name
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            batched()
        torch.cuda.synchronize()
    kernels = {}
    for e in prof.key_averages():
        t = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
        if t > 0:
            kernels[e.key.split('(')[0].split('::')[-1][:60]] = t / 20
    sel = sum(v for k, v in kernels.items() if 'topk_hist' in k or 'topk_compact' in k)
    # worst case of the exact stage: every score of level 0 equal (2.7 M keys in one bin, per image)
    cls_eq = [torch.full_like(cls[0], 0.5)] + cls[1:]
    t_eq = timeit(lambda: S.sph_get_bboxes(cls_eq, box, anchors, bbox_coder=coder_, score_thr=0.05, nms_pre=1000, nms=nms, max_per_img=100,
                                           iou_calculator='sph2pob_efficient', box_version=4, activation='none'), warm=2, reps=5) * 1e6
    return {'config': 'get_bboxes: %d images x 98208 anchors x 37 classes (512x1024 ERP, NCHW), nms_pre 1000, max_per_img 100' % images,
            'a_batched_eager_us': med(ta), 'b_batched_graph_us': med(tb), 'c_per_image_loop_us': med(tc),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'a_spread_us': max(ta) - min(ta), 'b_spread_us': max(tb) - min(tb),
            'c_spread_us': max(tc) - min(tc), 'a_over_c': med(ta) / med(tc), 'b_over_c': med(tb) / med(tc),
            'score_bytes': score_bytes, 'copy_bandwidth_TBps': bw / 1e12, 'stream_floor_us_one_pass': score_bytes / bw * 1e6,
            'stream_floor_us_two_passes': 2 * score_bytes / bw * 1e6, 'num_dets': r.num_dets.tolist(),
            'kernel_us': kernels, 'selection_streams_us': sel, 'selection_over_two_pass_floor': sel / (2 * score_bytes / bw * 1e6) if sel else None,
            'all_equal_level0_eager_us': t_eq,
            'note': 'kernel_us: average device time per kernel name over 20 eager calls (torch device-activity trace); selection_streams_us '
                    '= topk_hist + topk_compact, the two passes over the scores'}


def focal(images=8, classes=37, rounds=7):
    """The classification loss of a minibatch (sph_focal_loss) at the reference's test shape — 512 x 1024 ERP, 5 levels, 9 anchors,
    37 classes, gamma 2, alpha 0.25, row weights, a device avg_factor — forward + backward on the head's NCHW logits: (a) eager;
    (b) the same replayed from a graph; (c) the torch composition a user runs without the kernel (permute / reshape / cat, the
    reference formula, sum / avg_factor; forward + backward).  Timed in alternation `rounds` times, medians and spreads reported.
    The fused kernel's device time is set against 2 x 4 x B n C bytes (each logit read once, each gradient written once) over
    the bandwidth of a device copy of the same tensors measured here (the method of tools/ubench/stream_floor.hip)."""
    import torch.nn.functional as F
    import demo_hot_path as D
    g = torch.Generator(device='cuda').manual_seed(0)
    cls = [(torch.randn((images, 9 * classes, h, w), generator=g, device='cuda') * 2 - 4).requires_grad_(True) for h, w in D.LEVEL_SHAPES]
    n = sum(9 * h * w for h, w in D.LEVEL_SHAPES)
    labels = torch.randint(0, classes, (images, n), generator=g, device='cuda')
    labels[torch.rand((images, n), generator=g, device='cuda') > 0.01] = classes      # ~1 % positives
    weights = (torch.rand((images, n), generator=g, device='cuda') > 0.02).float()
    avg = labels.ne(classes).sum().float().reshape(1)

    def fused():
        loss = S.sph_focal_loss(cls, labels, weights, gamma=2.0, alpha=0.25, avg_factor=avg)
        return (loss.detach(),) + torch.autograd.grad(loss, cls)

    def composition():
        x = torch.cat([c.permute(0, 2, 3, 1).reshape(images, -1, classes) for c in cls], 1).reshape(-1, classes)
        t = F.one_hot(labels.reshape(-1), classes + 1)[:, :classes].type_as(x)
        p = x.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        fw = (0.25 * t + 0.75 * (1 - t)) * pt.pow(2.0)
        loss = (F.binary_cross_entropy_with_logits(x, t, reduction='none') * fw * weights.reshape(-1, 1)).sum() / (avg + 1.1920929e-07)
        return (loss.detach().reshape(()),) + torch.autograd.grad(loss, cls)
    # the capture comes first, after a warm-up on a side stream, and nothing returned keeps an autograd graph alive (see bbox_loss)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused()
    a, c = fused(), composition()
    torch.cuda.synchronize()
    loss_rel = abs(float(a[0]) - float(c[0])) / abs(float(c[0]))
    grad_diff = max(float((x - y).abs().max()) for x, y in zip(a[1:], c[1:]))
    dst = [torch.empty_like(x) for x in cls]

    def copy():
        with torch.no_grad():
            for x, y in zip(dst, cls):
                x.copy_(y)
    ta, tb, tc, tcopy = [], [], [], []
    for _ in range(rounds):
        ta.append(timeit(fused, reps=30) * 1e6)
        tb.append(timeit(graph.replay, reps=30) * 1e6)
        tc.append(timeit(composition, warm=2, reps=5, settle_s=0.0) * 1e6)
        tcopy.append(timeit(copy, reps=30) * 1e6)
    med = lambda v: float(np.median(v))
    elems = images * n * classes
    stream_bytes = 2 * 4 * elems
    bw = stream_bytes / (med(tcopy) * 1e-6)   # a copy reads and writes each byte once: the same 2 x 4 x elems bytes
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            fused()
        torch.cuda.synchronize()
    kernels = {}
    for e in prof.key_averages():
        t = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
        if t > 0:
            kernels[e.key[:80]] = t / 20
    k_sum = sum(v for k, v in kernels.items() if 'focal_sum' in k)
    return {'config': 'focal: %d images x %d anchors x %d classes (512x1024 ERP, 5 NCHW levels), gamma 2, alpha 0.25, fwd + bwd' % (images, n, classes),
            'a_fused_eager_us': med(ta), 'b_fused_graph_us': med(tb), 'c_torch_composition_us': med(tc),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'a_spread_us': max(ta) - min(ta), 'b_spread_us': max(tb) - min(tb),
            'c_spread_us': max(tc) - min(tc), 'a_over_c': med(ta) / med(tc), 'b_over_c': med(tb) / med(tc),
            'elements': elems, 'stream_bytes': stream_bytes, 'copy_bandwidth_TBps': bw / 1e12, 'copy_floor_us': med(tcopy),
            'kernel_us': kernels, 'focal_sum_kernel_us': k_sum, 'focal_sum_kernel_TBps': stream_bytes / (k_sum * 1e-6) / 1e12 if k_sum else None,
            'focal_sum_over_copy_floor': k_sum / med(tcopy) if k_sum else None,
            'loss_fused': float(a[0]), 'loss_composition': float(c[0]), 'loss_rel_diff': loss_rel, 'grad_max_abs_diff': grad_diff,
            'note': 'kernel_us: average device time per kernel name over 20 eager calls (torch device-activity trace); the copy floor is a '
                    'device copy of the five logit tensors (reads and writes 4 B per element each, the bytes the fused kernel moves)'}


SSD300_LEVELS = ((4, 38, 38), (6, 19, 19), (6, 10, 10), (6, 5, 5), (4, 3, 3), (4, 1, 1))   # (A, H, W): 8 732 anchors


def softmax_mining(images=8, channels=38, rounds=7):
    """The softmax classification loss with hard-negative mining (sph_softmax_loss, neg_pos_ratio=3, row weights, a device
    avg_factor), forward + backward on the head's NCHW scores, at two shapes: the project's head (512 x 1024 ERP, 5 levels, 9
    anchors: 98 208 anchors) and SSD300's 8 732 anchors in 6 levels; K = 38 score channels at both.  Per shape: (a) eager; (b) the
    same replayed from a graph; (c) the torch composition of SphSSDHead.loss's classification half in this process — permute /
    reshape / cat, F.cross_entropy(reduction='none') * weights, then per image nonzero() twice, a host k and topk — forward +
    backward.  Timed in alternation `rounds` times, medians and spreads reported."""
    import torch.nn.functional as F
    import demo_hot_path as D
    shapes = (('head 512x1024 ERP, 5 levels', [(9, h, w) for h, w in D.LEVEL_SHAPES]), ('SSD300, 6 levels', list(SSD300_LEVELS)))
    med = lambda v: float(np.median(v))
    out = {'config': 'softmax_mining: %d images, K = %d, neg_pos_ratio 3, fwd + bwd' % (images, channels), 'shapes': []}
    for what, levels in shapes:
        g = torch.Generator(device='cuda').manual_seed(0)
        cls = [(torch.randn((images, a * channels, h, w), generator=g, device='cuda') * 2).requires_grad_(True) for a, h, w in levels]
        n = sum(a * h * w for a, h, w in levels)
        bg = channels - 1
        labels = torch.randint(0, bg, (images, n), generator=g, device='cuda')
        labels[torch.rand((images, n), generator=g, device='cuda') > 0.01] = bg      # ~1 % positives
        weights = (torch.rand((images, n), generator=g, device='cuda') > 0.02).float()
        avg = labels.ne(bg).sum().float().reshape(1)

        def fused():
            loss = S.sph_softmax_loss(cls, labels, weights, neg_pos_ratio=3, avg_factor=avg)
            return (loss.detach(),) + torch.autograd.grad(loss, cls)

        def forward_only():
            with torch.no_grad():
                return S.sph_softmax_loss(cls, labels, weights, neg_pos_ratio=3, avg_factor=avg)

        def composition():
            x = torch.cat([c.permute(0, 2, 3, 1).reshape(images, -1, channels) for c in cls], 1)
            total = x.new_zeros(())
            for b in range(images):
                loss_all = F.cross_entropy(x[b], labels[b], reduction='none') * weights[b]
                pos = ((labels[b] >= 0) & (labels[b] < bg)).nonzero(as_tuple=False).reshape(-1)
                neg = (labels[b] == bg).nonzero(as_tuple=False).reshape(-1)
                k = min(3 * pos.size(0), neg.size(0))
                top, _ = loss_all[neg].topk(k)
                total = total + loss_all[pos].sum() + top.sum()
            loss = total / (avg + 1.1920929e-07)
            return (loss.detach().reshape(()),) + torch.autograd.grad(loss, cls)
        # The capture comes first, after a warm-up on a side stream, and nothing returned keeps an autograd graph alive (see
        # _decoded_loss: a gradient edge of `cls` left by an eager call on the default stream invalidates the capture).
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fused()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused()
        a, c = fused(), composition()
        torch.cuda.synchronize()
        loss_rel = abs(float(a[0]) - float(c[0])) / abs(float(c[0]))
        grad_diff = max(float((x - y).abs().max()) for x, y in zip(a[1:], c[1:]))
        ta, tb, tc, tf = [], [], [], []
        for _ in range(rounds):
            ta.append(timeit(fused, reps=30) * 1e6)
            tb.append(timeit(graph.replay, reps=30) * 1e6)
            tc.append(timeit(composition, warm=2, reps=5, settle_s=0.0) * 1e6)
            tf.append(timeit(forward_only, reps=30) * 1e6)
        out['shapes'].append({
            'shape': '%s: %d anchors' % (what, n), 'a_fused_eager_us': med(ta), 'b_fused_graph_us': med(tb), 'c_torch_composition_us': med(tc),
            'f_fused_forward_only_us': med(tf),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'f_rounds_us': tf, 'a_spread_us': max(ta) - min(ta),
            'b_spread_us': max(tb) - min(tb), 'c_spread_us': max(tc) - min(tc), 'f_spread_us': max(tf) - min(tf),
            'a_over_c': med(ta) / med(tc), 'b_over_c': med(tb) / med(tc), 'logit_bytes': 4 * images * n * channels,
            'loss_fused': float(a[0]), 'loss_composition': float(c[0]), 'loss_rel_diff': loss_rel, 'grad_max_abs_diff': grad_diff})
        del graph
    out['note'] = ('f: the forward alone under no_grad (rows -> keys, cut, final: no gradient pass).  The composition synchronises with '
                   'the host twice per image (nonzero) and cannot be captured.')
    return out


def _decoded_loss(name, what, fused_loss, module, images_counts, classes, rounds):
    """The scene and the four timings shared by bbox_loss and gauss_bbox_loss: `fused_loss(preds, anchors, t, coder)` is the fused
    call, `module` the loss module of the composition."""
    import demo_hot_path as D
    images = len(images_counts)
    g = torch.Generator().manual_seed(0)
    anchors = torch.cat(D.retina_level_anchors())
    gts, labels = [], []
    for k in images_counts:
        u = torch.rand((k, 4), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda())
        labels.append(torch.randint(0, classes, (k,), generator=g).cuda())
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4))
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    t = S.sph_anchor_targets(anchors, gts, labels, assigner=assigner, num_classes=classes)
    n = anchors.size(0)
    rois = anchors.repeat(images, 1)
    targets2, weights2 = t.bbox_targets.reshape(-1, 4), t.bbox_weights.reshape(-1, 4)
    gd = torch.Generator(device='cuda').manual_seed(0)
    preds = [(torch.randn((images, 9 * 4, h, w), generator=gd, device='cuda') * 0.05).requires_grad_(True) for h, w in D.LEVEL_SHAPES]

    def fused():
        loss = fused_loss(preds, anchors, t, coder)
        return (loss.detach(),) + torch.autograd.grad(loss, preds)

    def composition():
        flat = torch.cat([p.permute(0, 2, 3, 1).reshape(images, -1, 4) for p in preds], 1).reshape(-1, 4)
        loss = module(coder.decode(rois, flat), targets2, weights2, avg_factor=t.avg_factor)
        return (loss.detach().reshape(()),) + torch.autograd.grad(loss, preds)
    # The captures come first, each after a warm-up on a side stream, and nothing returned keeps an autograd graph alive: a
    # gradient edge of `preds` created by an eager call on the default stream and still alive at capture time makes autograd
    # synchronise with the default stream inside the capture, which invalidates it (tools/graph_capture_backward.py, 'stale').
    graphs = []
    for fn in (fused, composition):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graphs.append(graph)
    a, c = fused(), composition()
    torch.cuda.synchronize()
    loss_rel = abs(float(a[0]) - float(c[0])) / abs(float(c[0]))
    grad_diff = max(float((x - y).abs().max()) for x, y in zip(a[1:], c[1:]))
    ta, tb, tc, td = [], [], [], []
    for _ in range(rounds):
        ta.append(timeit(fused, reps=30) * 1e6)
        tb.append(timeit(graphs[0].replay, reps=30) * 1e6)
        tc.append(timeit(composition, reps=30) * 1e6)
        td.append(timeit(graphs[1].replay, reps=30) * 1e6)
    med = lambda v: float(np.median(v))
    return {'config': '%s: %d images x %d anchors (512x1024 ERP, 5 NCHW levels), %s, device avg_factor, fwd + bwd' % (name, images, n, what),
            'num_gt': list(images_counts), 'num_pos': t.num_pos.tolist(),
            'a_fused_eager_us': med(ta), 'b_fused_graph_us': med(tb), 'c_composition_eager_us': med(tc), 'd_composition_graph_us': med(td),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'd_rounds_us': td,
            'a_spread_us': max(ta) - min(ta), 'b_spread_us': max(tb) - min(tb), 'c_spread_us': max(tc) - min(tc), 'd_spread_us': max(td) - min(td),
            'a_over_c': med(ta) / med(tc), 'b_over_d': med(tb) / med(td),
            'loss_fused': float(a[0]), 'loss_composition': float(c[0]), 'loss_rel_diff': loss_rel, 'grad_max_abs_diff': grad_diff}


def bbox_loss(images_counts=(64, 1, 0, 17, 64, 3, 128, 33), classes=37, rounds=7):
    """The regression loss of a minibatch at the reference's test shape — 512 x 1024 ERP, 5 NCHW levels, 9 anchors, 98 208 anchors
    per image, the ground-truth counts of demo_hot_path.run_batch, CIoU, a device avg_factor — forward + backward to the head's
    NCHW deltas: (a) sph_bbox_loss eager, (b) replayed from a graph, (c) the composition it replaces (permute / reshape / cat ->
    coder.decode -> Sph2PobIoULoss -> / avg_factor) eager and (d) replayed from a graph.  Timed in alternation `rounds` times,
    medians and spreads reported."""
    return _decoded_loss('bbox_loss', 'CIoU', lambda preds, anchors, t, coder: S.sph_bbox_loss(
        preds, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='ciou', avg_factor=t.avg_factor),
        Sph2PobIoULoss(mode='ciou', loss_weight=1.0), images_counts, classes, rounds)


def gauss_bbox_loss(images_counts=(64, 1, 0, 17, 64, 3, 128, 33), classes=37, rounds=7):
    """bbox_loss with loss_bbox = Sph2PobGDLoss(kld): (a) sph_gauss_bbox_loss eager, (b) replayed from a graph, (c) the composition
    it replaces (permute / reshape / cat -> coder.decode -> Sph2PobGDLoss -> / avg_factor) eager and (d) replayed from a graph."""
    from sph_retina_amd.losses.sph2pob_gaussian_loss import Sph2PobGDLoss
    module = Sph2PobGDLoss(loss_type='kld', loss_weight=1.0)
    return _decoded_loss('gauss_bbox_loss', 'Sph2PobGDLoss kld', lambda preds, anchors, t, coder: S.sph_gauss_bbox_loss(
        preds, anchors, t.bbox_targets, t.bbox_weights, bbox_coder=coder, loss=module, avg_factor=t.avg_factor),
        module, images_counts, classes, rounds)


def delta_loss(images_counts=(64, 1, 0, 17, 64, 3, 128, 33), classes=37, rounds=7):
    """The regression loss of the reference's BASE configuration (L1Loss on encoded deltas, reg_decoded_bbox=False) for a minibatch
    at the reference's test shape — 512 x 1024 ERP, 5 NCHW levels, 9 anchors, 98 208 anchors per image, the ground-truth counts of
    demo_hot_path.run_batch, a device avg_factor — forward + backward to the head's NCHW deltas: (a) sph_delta_loss eager, (b)
    replayed from a graph, (c) the composition it replaces (permute / reshape / cat -> |pred - target| * weight -> sum /
    (avg_factor + eps)) eager and (d) replayed from a graph.  Timed in alternation `rounds` times, medians and spreads reported."""
    import demo_hot_path as D
    images = len(images_counts)
    g = torch.Generator().manual_seed(0)
    anchors = torch.cat(D.retina_level_anchors())
    gts, labels = [], []
    for k in images_counts:
        u = torch.rand((k, 4), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda())
        labels.append(torch.randint(0, classes, (k,), generator=g).cuda())
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4))
    coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.))
    t = S.sph_anchor_targets(anchors, gts, labels, assigner=assigner, num_classes=classes, reg_decoded_bbox=False, bbox_coder=coder)
    n = anchors.size(0)
    eps = float(torch.finfo(torch.float32).eps)
    gd = torch.Generator(device='cuda').manual_seed(0)
    preds = [(torch.randn((images, 9 * 4, h, w), generator=gd, device='cuda') * 0.05).requires_grad_(True) for h, w in D.LEVEL_SHAPES]

    def fused():
        loss = S.sph_delta_loss(preds, t.bbox_targets, t.bbox_weights, avg_factor=t.avg_factor)
        return (loss.detach(),) + torch.autograd.grad(loss, preds)

    def composition():
        flat = torch.cat([p.permute(0, 2, 3, 1).reshape(images, -1, 4) for p in preds], 1)
        loss = ((flat - t.bbox_targets).abs() * t.bbox_weights).sum() / (t.avg_factor.reshape(()) + eps)
        return (loss.detach().reshape(()),) + torch.autograd.grad(loss, preds)
    # the captures come first, each after a warm-up on a side stream (see bbox_loss above)
    graphs = []
    for fn in (fused, composition):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graphs.append(graph)
    a, c = fused(), composition()
    torch.cuda.synchronize()
    loss_rel = abs(float(a[0]) - float(c[0])) / abs(float(c[0]))
    grad_diff = max(float((x - y).abs().max()) for x, y in zip(a[1:], c[1:]))
    ta, tb, tc, td = [], [], [], []
    for _ in range(rounds):
        ta.append(timeit(fused, reps=30) * 1e6)
        tb.append(timeit(graphs[0].replay, reps=30) * 1e6)
        tc.append(timeit(composition, reps=30) * 1e6)
        td.append(timeit(graphs[1].replay, reps=30) * 1e6)
    med = lambda v: float(np.median(v))
    return {'config': 'delta_loss: %d images x %d anchors (512x1024 ERP, 5 NCHW levels), L1 on encoded deltas, device avg_factor, fwd + bwd' % (images, n),
            'num_gt': list(images_counts), 'num_pos': t.num_pos.tolist(),
            'a_fused_eager_us': med(ta), 'b_fused_graph_us': med(tb), 'c_composition_eager_us': med(tc), 'd_composition_graph_us': med(td),
            'a_rounds_us': ta, 'b_rounds_us': tb, 'c_rounds_us': tc, 'd_rounds_us': td,
            'a_spread_us': max(ta) - min(ta), 'b_spread_us': max(tb) - min(tb), 'c_spread_us': max(tc) - min(tc), 'd_spread_us': max(td) - min(td),
            'a_over_c': med(ta) / med(tc), 'b_over_d': med(tb) / med(td),
            'loss_fused': float(a[0]), 'loss_composition': float(c[0]), 'loss_rel_diff': loss_rel, 'grad_max_abs_diff': grad_diff}


def coder(n=1_000_000):
    """§8f-2: decode (the op in front of loss_bbox) and encode on n RBFoV / BFoV boxes, via the C ABI."""
    import ctypes
    from sph_retina_amd import _lib, _torch_glue as G
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {'config': 'box coder, %d boxes (sph2pob_coder_*_f32 through the C ABI)' % n}
    for dim in (4, 5):
        a, g = boxes(n, 3, dim).contiguous(), boxes(n, 4, dim).contiguous()
        d = torch.randn((n, dim), device='cuda')
        o, go = torch.empty_like(d), torch.randn((n, dim), device='cuda')
        stds = (ctypes.c_float * dim)(*([0.1, 0.1, 0.2, 0.2, 0.1][:dim]))
        nn, mr = ctypes.c_int64(n), ctypes.c_float(abs(math.log(16 / 1000)))
        te = timeit(lambda: lib.sph2pob_coder_encode_f32(G.ptr(a), G.ptr(g), None, stds, G.ptr(o), nn, dim, st), reps=100)
        td = timeit(lambda: lib.sph2pob_coder_decode_f32(G.ptr(a), G.ptr(d), None, stds, G.ptr(o), nn, 1, dim, mr, 1,
                                                         ctypes.c_float(32), st), reps=100)
        tb = timeit(lambda: lib.sph2pob_coder_decode_bwd_f32(G.ptr(a), G.ptr(d), G.ptr(go), None, stds, G.ptr(o), nn, 1, dim,
                                                             mr, 1, ctypes.c_float(32), st), reps=100)
        bpb = 4 * dim
        out['dim%d' % dim] = {'encode_us': te * 1e6, 'decode_us': td * 1e6, 'decode_bwd_us': tb * 1e6,
                              'bytes_per_box': {'encode': 3 * bpb, 'decode': 3 * bpb, 'decode_bwd': 4 * bpb},
                              'hbm_GBps': {'encode': 3 * bpb * n / te / 1e9, 'decode': 3 * bpb * n / td / 1e9,
                                           'decode_bwd': 4 * bpb * n / tb / 1e9}}
    return out


def unbiased(n=1_000_000):
    """§8f-4: Unbiased IoU (fp64 spherical-polygon area) on the benchmark's uniform pairs, aligned; plus the CPU
    restatement timed on a bounded sample for scale (README quotes 46 s per 1 M pairs for the reference's numpy)."""
    from sph_retina_amd.iou import naive_iou, unbiased_iou
    out = {'config': 'unbiased_iou / naive_iou, %d aligned pairs' % n}
    for dim in (4, 5):
        a, b = boxes(n, 0, dim), boxes(n, 1, dim)
        near = a + torch.randn_like(a) * 4
        near[:, 1].clamp_(1, 179)
        near[:, 2:4].clamp_(1, 170)
        tu = timeit(lambda: unbiased_iou(a, b, is_aligned=True), reps=20)
        tn = timeit(lambda: unbiased_iou(a, near, is_aligned=True), reps=20)
        tv = timeit(lambda: naive_iou(a, b, is_aligned=True), reps=50)
        out['dim%d' % dim] = {'unbiased_uniform_us': tu * 1e6, 'unbiased_uniform_pairs_per_s': n / tu,
                              'unbiased_nearby_us': tn * 1e6, 'unbiased_nearby_pairs_per_s': n / tn,
                              'naive_uniform_us': tv * 1e6}
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import oracle as O
        m = 200_000
        a, b = boxes(m, 0, 4).cpu().numpy(), boxes(m, 1, 4).cpu().numpy()
        O.unbiased_iou(a[:1000], b[:1000])
        t0 = time.perf_counter()
        O.unbiased_iou(a, b)
        dt = time.perf_counter() - t0
        out['cpu_restatement_pairs_per_s'] = m / dt
        out['cpu_threads'] = O.max_threads()
    except Exception as e:  # the oracle is test infrastructure; its absence must not break the GPU numbers
        out['cpu_restatement_error'] = repr(e)
    return out


def variants(n=1_000_000):
    """Aligned IoU, 1 M uniform pairs, every operator of sphdet.iou that the kernels serve (us per call through the
    Python boundary, back-to-back)."""
    from sph_retina_amd import iou as I
    out = {'config': 'aligned IoU operators, %d uniform pairs (us per call)' % n}
    for dim in (4, 5):
        a, b = boxes(n, 0, dim), boxes(n, 1, dim)
        ops = [('sph2pob_standard_iou', I.sph2pob_standard_iou), ('sph2pob_efficient_iou', I.sph2pob_efficient_iou)]
        if dim == 4:
            ops += [('sph2pob_legacy_iou', I.sph2pob_legacy_iou), ('sph_iou', I.sph_iou), ('fov_iou', I.fov_iou)]
        r = {}
        for name, fn in ops:
            r[name] = timeit(lambda: fn(a, b, is_aligned=True), warm=50, reps=300) * 1e6
        out['bfov' if dim == 4 else 'rbfov'] = r
    return out


def gaussian(n=1_000_000):
    """Sph2PobGDLoss (kld) and Sph2PobKFLoss forward+backward on config3's 1 M RBFoV pairs, through autograd and through the C
    ABI (fwd_grad + final sum + grad_scale, as the autograd Function launches), timed beside the CIoU step."""
    import ctypes
    from sph_retina_amd import _lib, _torch_glue as G
    from sph_retina_amd.losses import Sph2PobGDLoss, Sph2PobKFLoss
    tgt = boxes(n, 0, 5, alpha=(5, 90), gamma=(-60, 60))
    g = torch.Generator().manual_seed(1)
    pred = tgt + (torch.randn((n, 5), generator=g) * torch.tensor([8., 8., 6., 6., 10.])).cuda()
    pred[:, 0] %= 360
    pred[:, 1].clamp_(1, 179)
    pred[:, 2:4].clamp_(1, 170)
    pred.requires_grad_(True)
    lib = _lib.lib()
    p_, t_ = pred.detach().contiguous(), tgt.contiguous()
    out, one = torch.empty((), device='cuda'), torch.ones((), device='cuda')
    ws2 = torch.empty(lib.sph2pob_loss_sum_workspace_floats(n), device='cuda')
    stash = torch.empty_like(p_)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nn, null = ctypes.c_int64(n), ctypes.c_void_p(0)
    res = {'config': 'configs[2] pairs (1,000,000 RBFoV), Sph2PobGDLoss / Sph2PobKFLoss forward+backward', 'pairs': n}
    ciou = Sph2PobIoULoss(mode='ciou', reduction='mean')

    def ciou_abi():
        lib.sph2pob_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null, ctypes.c_void_p(out.data_ptr()),
                                      G.ptr(ws2), G.ptr(stash), null, nn, 5, 3, ctypes.c_float(1e-6), st)
        lib.sph2pob_loss_grad_scale_f32(G.ptr(stash), ctypes.c_void_p(one.data_ptr()), 0, G.ptr(stash), nn, 5, st)

    def ciou_step():
        pred.grad = None
        ciou(pred, tgt).backward()
    res['ciou_c_abi_fwd_bwd_ms'] = timeit(ciou_abi) * 1e3
    res['ciou_autograd_fwd_bwd_ms'] = timeit(ciou_step) * 1e3
    # (name, module, C-ABI trailing arguments: type, fun, tau, alpha, opts, beta, eps)
    for name, mod, tail in (('kld', Sph2PobGDLoss(loss_type='kld'), (1, 1, 0.0, 1.0, 1, 1 / 9, 1e-6)),
                            ('gwd', Sph2PobGDLoss(loss_type='gwd'), (0, 1, 0.0, 1.0, 2, 1 / 9, 1e-6)),
                            ('kf', Sph2PobKFLoss(), (5, 0, 0.0, 1.0, 0, 1 / 9, 1e-6))):
        ct = (ctypes.c_int(tail[0]), ctypes.c_int(tail[1]), ctypes.c_float(tail[2]), ctypes.c_float(tail[3]), ctypes.c_int(tail[4]),
              ctypes.c_float(tail[5]), ctypes.c_float(tail[6]))

        def abi():
            lib.sph2pob_gauss_loss_fwd_grad_f32(G.ptr(p_), G.ptr(t_), null, 0, ctypes.c_float(1.0 / n), null,
                                                ctypes.c_void_p(out.data_ptr()), G.ptr(ws2), G.ptr(stash), null, nn, 5, *ct, st)
            lib.sph2pob_loss_grad_scale_f32(G.ptr(stash), ctypes.c_void_p(one.data_ptr()), 0, G.ptr(stash), nn, 5, st)

        def step():
            pred.grad = None
            mod(pred, tgt).backward()
        ta = timeit(abi)
        res[f'{name}_c_abi_fwd_bwd_ms'] = ta * 1e3
        res[f'{name}_autograd_fwd_bwd_ms'] = timeit(step) * 1e3
        res[f'{name}_roofline'] = pmc_roofline('loss_fwd_grad_kernel', ta, 60.0 * n, gauss=True)
    res['note'] = ('c_abi = gauss_loss_fwd_grad (forward + gradients + partial sums in one pass) + final sum + grad_scale (in '
                   'place, g = 1); roofline at 60 B/pair (pred, target, grad_pred)')
    return res


if __name__ == '__main__':
    # config4 twice: the reference's default 512 x 1024 ERP (98 208 anchors: the "~100k" of BASELINE configs[3]) and the
    # literal 1024 x 2048 grid (392 832 anchors, SURVEY §8d "secondary")
    # (arguments select configurations by name: config3 gaussian config4 config4b config4_batch train_targets get_bboxes focal softmax_mining bbox_loss gauss_bbox_loss delta_loss coder unbiased variants; none = all)
    table = dict(config3=config3, gaussian=gaussian, config4=config4, config4b=lambda: config4(1024, 2048), config4_batch=config4_batch, train_targets=train_targets, get_bboxes=get_bboxes, focal=focal, softmax_mining=softmax_mining, bbox_loss=bbox_loss, gauss_bbox_loss=gauss_bbox_loss, delta_loss=delta_loss, coder=coder, unbiased=unbiased,
                 variants=variants)
    for name in (sys.argv[1:] or list(table)):
        print(json.dumps(table[name]()), flush=True)
