"""python tools/time_fcos_losses.py [OUT.jsonl] — the fused regression and centerness losses of an FCOS head at B = 8, P = 10 912
(512 x 1024, strides 8 ... 128), 20 GT per image, forward + backward to the head's NCHW leaves, each against the torch composition
it replaces on the same GPU (tools/demo_hot_path.fcos_step):
    bbox   sph_point_bbox_loss                       | permute / reshape / cat, two coder.decode, Sph2PobIoULoss over all B P rows
    bce    sph_bce_loss on the centerness levels     | permute / reshape / cat, binary_cross_entropy_with_logits, mask, sum, divide
    step   fcos_step(fused_losses=True)              | fcos_step: sph_fcos_targets + sph_focal_loss + the two compositions
The targets are computed once outside the timed region for `bbox` and `bce`, inside it for `step`.  Each side is timed eager and as
a replay of its captured graph (all graphs are captured first, before any eager call keeps an autograd graph alive: DESIGN.md 4.8).
Device events around brackets of LAUNCHES calls, median / p10 / p90 of the per-call time over the brackets; the four alternate in
blocks.  `--profile`: a short untimed run of every side for `rocprofv3 --kernel-trace --stats`."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import sph_retina_amd as S  # noqa: E402
from demo_hot_path import FCOS_CFG, LEVEL_SHAPES, fcos_head_outputs, fcos_step  # noqa: E402

BRACKETS, WARM, BLOCK, LAUNCHES = int(os.environ.get('BRACKETS', 60)), 3, 10, 10
B, K, C = 8, 20, 37
PROFILE = '--profile' in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith('--')]
out = open(args[0], 'w') if args else None   # the JSON lines, also printed (profiles/fcos_losses_bench.jsonl)


def timed(fn, brackets, launches):
    ts = []
    for _ in range(brackets):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / launches)
    return ts


def stats(ts, launches):
    ts = sorted(ts)
    return dict(median_us=round(statistics.median(ts), 1), p10_us=round(ts[len(ts) // 10], 1), p90_us=round(ts[len(ts) * 9 // 10], 1),
                brackets=len(ts), launches_per_bracket=launches)


def captured(fn):
    """fn as a graph replay: warmed on a side stream, then captured once."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph, keep


assert torch.cuda.is_available(), 'time_fcos_losses.py measures on an MI355X: there is no CPU figure'
dim = 4
points = S.sph_fcos_points(LEVEL_SHAPES, FCOS_CFG['strides'], device='cuda')
pts = torch.cat(points)
g = torch.Generator().manual_seed(0)
u = torch.rand((B * K, 5), generator=g)
gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85, u[:, 4] * 90], 1)[:, :dim].contiguous().cuda()
labels = torch.randint(0, C, (B * K,), generator=g).cuda()
offsets = (torch.arange(B + 1, dtype=torch.int64) * K).cuda()
cls, box, ctr = fcos_head_outputs(B, C, dim, 0, 'cuda')
coder, loss_iou = S.DistancePointSphBBoxCoder(box_version=dim), S.Sph2PobIoULoss(mode='iou')
kw = dict(FCOS_CFG, num_classes=C, coder=coder, loss_iou=loss_iou, img_shape=(512, 1024), k_max=K)
t = S.sph_fcos_targets(points, gt, labels, offsets, num_classes=C, img_shape=(512, 1024), k_max=K, **FCOS_CFG)
pos = (t.labels < C).float()
eps = torch.finfo(torch.float32).eps


def bbox_fused():
    loss = S.sph_point_bbox_loss(box, points, t.bbox_targets, t.bbox_weights, bbox_coder=coder, mode='iou', avg_factor=t.centerness_denorm)
    return (loss,) + torch.autograd.grad(loss, box)


def bbox_composition():
    flat = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, dim) for p in box], dim=1)
    loss = loss_iou(coder.decode(pts, flat).reshape(-1, dim), coder.decode(pts, t.bbox_targets).reshape(-1, dim), t.centerness_targets.reshape(-1),
                    avg_factor=t.centerness_denorm)
    return (loss,) + torch.autograd.grad(loss, box)


def bce_fused():
    loss = S.sph_bce_loss(ctr, t.centerness_targets, pos, avg_factor=t.avg_factor)
    return (loss,) + torch.autograd.grad(loss, ctr)


def bce_composition():
    flat = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1) for c in ctr], dim=1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(flat, t.centerness_targets, reduction='none')
    loss = (bce * pos).sum() / (t.avg_factor + eps)
    return (loss,) + torch.autograd.grad(loss, ctr)


def step(fused):
    def run():
        a, b, c, _ = fcos_step(points, gt, labels, offsets, cls, box, ctr, fused_losses=fused, **kw)
        return (a, b, c) + torch.autograd.grad(a + b + c, cls + box + ctr)
    return run


CASES = (('bbox', bbox_fused, bbox_composition), ('bce', bce_fused, bce_composition), ('step', step(True), step(False)))
if PROFILE:
    for name, fused, comp in CASES:
        for fn in (fused, comp):
            for _ in range(20):
                fn()
    torch.cuda.synchronize()
    sys.exit(0)

graphs = {}
for name, fused, comp in CASES:   # every capture before the first timed eager call
    graphs[name] = (captured(fused), captured(comp))
for name, fused, comp in CASES:
    (gf, keep_f), (gc, keep_c) = graphs[name]
    sides = (('fused_eager', fused), ('composition_eager', comp), ('fused_graph', gf.replay), ('composition_graph', gc.replay))
    for _, fn in sides:
        timed(fn, WARM, LAUNCHES)
    ts = {k: [] for k, _ in sides}
    for _ in range(BRACKETS // BLOCK):
        for k, fn in sides:
            ts[k] += timed(fn, BLOCK, LAUNCHES)
    gf.replay()
    gc.replay()
    torch.cuda.synchronize()
    line = dict(case=name, images=B, points=t.labels.size(1), gt_per_image=K, box_dim=dim, positives=int(t.num_pos.sum()),
                **{k: stats(v, LAUNCHES) for k, v in ts.items()},
                losses_fused=[float(x.detach()) for x in keep_f[:3 if name == 'step' else 1]],
                losses_composition=[float(x.detach()) for x in keep_c[:3 if name == 'step' else 1]])
    print(json.dumps(line), flush=True)
    if out is not None:
        out.write(json.dumps(line) + '\n')
        out.flush()
