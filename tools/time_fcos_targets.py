"""python tools/time_fcos_targets.py [OUT.jsonl] — sph_fcos_targets at B = 8, P = 10 912 (512 x 1024, strides 8 ... 128), 20 GT per
image, against the per-image torch composition of the reference on the same GPU (tests/fcos_targets_restatement.get_targets: the
reference's _get_target_single per image, the level-major concatenation, centerness_target and the two normalisers, which it reads
back to the host as the reference does).  Both produce the targets, the centerness targets and the two normalisers.
Device events around brackets of LAUNCHES calls (the batched call is a few tens of microseconds: one event pair per call would time
the events), median / p10 / p90 of the per-call time over the brackets; the two alternate in blocks."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import sph_retina_amd as S  # noqa: E402
from demo_hot_path import FCOS_CFG, LEVEL_SHAPES  # noqa: E402
from fcos_targets_restatement import get_targets  # noqa: E402

BRACKETS, WARM, BLOCK, LAUNCHES = int(os.environ.get('BRACKETS', 60)), 5, 10, 20
B, K, C = 8, 20, 80
out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None   # the JSON lines, also printed (profiles/fcos_targets_bench.jsonl)


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


assert torch.cuda.is_available(), 'time_fcos_targets.py measures on an MI355X: there is no CPU figure'
points = S.sph_fcos_points(LEVEL_SHAPES, FCOS_CFG['strides'], device='cuda')
g = torch.Generator().manual_seed(0)
for dim, center_sampling, norm_on_bbox in ((4, False, False), (4, True, True), (5, True, True)):
    u = torch.rand((B * K, 5), generator=g)
    gt = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85, u[:, 4] * 90], 1)[:, :dim].contiguous().cuda()
    labels = torch.randint(0, C, (B * K,), generator=g).cuda()
    offsets = (torch.arange(B + 1, dtype=torch.int64) * K).cuda()
    gts, labs = list(gt.split(K)), list(labels.split(K))
    kw = dict(FCOS_CFG, num_classes=C, box_version=dim, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, img_shape=(512, 1024))

    def batched():
        return S.sph_fcos_targets(points, gt, labels, offsets, k_max=K, **kw)

    def per_image():
        return get_targets(points, gts, labs, **kw)
    timed(batched, WARM, LAUNCHES)
    timed(per_image, WARM, 1)
    tb, tp = [], []
    for _ in range(BRACKETS // BLOCK):
        tb += timed(batched, BLOCK, LAUNCHES)
        tp += timed(per_image, BLOCK, 1)
    r, w = batched(), per_image()
    # (informational: on the GPU torch divides by a scalar as a product with its reciprocal, so its composition need not have the
    # bits of the CPU composition the library is held to; the tests compare against the CPU)
    same = [bool(torch.equal(r.labels, w.labels)), bool(torch.equal(r.bbox_targets.view(torch.int32), w.bbox_targets.view(torch.int32)))]
    line = dict(box_dim=dim, center_sampling=center_sampling, norm_on_bbox=norm_on_bbox, images=B, points=r.labels.size(1), gt_per_image=K,
                batched=stats(tb, LAUNCHES), per_image_composition=stats(tp, 1), num_pos=r.num_pos.tolist(), avg_factor=float(r.avg_factor),
                centerness_denorm=float(r.centerness_denorm), same_labels_as_gpu_composition=same[0], same_target_bits_as_gpu_composition=same[1], launches_batched=2, host_reads_batched=0)
    print(json.dumps(line), flush=True)
    if out is not None:
        out.write(json.dumps(line) + '\n')
        out.flush()
