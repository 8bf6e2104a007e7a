"""python tools/time_fcos_bboxes.py [OUT.jsonl] — sph_fcos_bboxes at B = 8, the real FCOS shape (strides 8 ... 128 on 512 x 1024:
10 912 points, C = 37), nms_pre = 1000, under the PANDORA configuration and the base planar one, for fp32 and bfloat16 levels:
  (i)   batched     sph_fcos_bboxes on the head's logits
  (ii)  per_image   the per-image composition of tests/fcos_bboxes_restatement.py on each image (torch sigmoid, stable sort,
                    DistancePointSphBBoxCoder.decode, the gather of the factor, the fp32 product, sph_batched_nms / PlanarNMS): what the
                    parent commit offers an FCOS head
  (iii) sibling     sph_test_bboxes on the SAME class logits with a delta coder and 10 912 anchors: the same pipeline without the
                    centerness gather and with the other decode (its boxes, and so its NMS load, are its own)
Device events around each step, median / p10 / p90 over settled steps; the sides alternate in blocks.  (An event bracket with a
synchronise per step adds the launch latency of the first kernel to every figure alike; the differences are not affected.)

python tools/time_fcos_bboxes.py --profile — (i) and (iii) alone, fp32, PANDORA, 40 calls each and no events: the program
of a `rocprofv3 --kernel-trace --stats` run of its own (cand_build_kernel<PointSource> beside cand_build_kernel<DeltaSource>).

python tools/time_fcos_bboxes.py --split KERNEL_TRACE.csv KERNEL_STATS.csv OUT_STATS.csv OUT_SPLIT.json — needs no GPU: from that
run's kernel trace, the average device time of each of the library's kernels per call and side (a call begins at its zero_kernel;
the first 40 calls are (i), the rest (iii); the first 5 calls of each side are left out), and the library's rows of its kernel
statistics (profiles/fcos_bboxes_kernel_split.json, profiles/fcos_bboxes_kernel_stats.csv)."""
import collections
import csv
import json
import os
import statistics
import sys

PROFILE_CALLS, PROFILE_SKIP = 40, 5
# what a kernel's name holds -> its stage, the first match counts: cand_build_kernel<Source> is told apart by its candidate source,
# and a trace of a build that still had cand_build_points_kernel reads the same (the stage names are those of the recorded
# profiles/fcos_bboxes_kernel_split.json)
STAGES = {'zero_kernel': 'zero_kernel', 'topk_hist': 'topk_hist', 'topk_cut': 'topk_cut', 'topk_compact': 'topk_compact', 'topk_resolve': 'topk_resolve',
          'PointSource': 'cand_build_points', 'cand_build_points': 'cand_build_points', 'cand_build': 'cand_build', 'nms_prepare': 'nms_prepare', 'nms_mask_compact': 'nms_mask_compact',
          'nms_sweep': 'nms_sweep', 'nms_select': 'nms_select'}


def ours(name):
    """A kernel of the library: in its anonymous namespace, and none of torch's."""
    return 'anonymous namespace)::' in name and 'at::native' not in name


def split_trace(trace_csv, stats_csv, out_stats, out_split):
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r['Start_Timestamp']))
    calls = []
    for r in rows:
        if not ours(r['Kernel_Name']):
            continue
        if 'zero_kernel' in r['Kernel_Name']:
            calls.append([])
        if calls:
            stage = next(stage for needle, stage in STAGES.items() if needle in r['Kernel_Name'])
            calls[-1].append((stage, int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    assert len(calls) == 2 * PROFILE_CALLS, len(calls)
    split = dict(source='rocprofv3 --kernel-trace --stats -- python tools/time_fcos_bboxes.py --profile (fp32, PANDORA, B = 8, 10 912 points; '
                        f'{PROFILE_CALLS} calls per side, the first {PROFILE_SKIP} of each side left out); average device time per kernel and call '
                        'in microseconds, the trace split at the calls\' first kernel')
    for side, chunk in (('sph_fcos_bboxes', calls[:PROFILE_CALLS]), ('sph_test_bboxes_sibling', calls[PROFILE_CALLS:])):
        per = collections.defaultdict(list)
        for call in chunk[PROFILE_SKIP:]:
            for stage, ns in call:
                per[stage].append(ns)
        avg = {stage: round(sum(v) / len(v) / 1e3, 1) for stage, v in per.items()}
        split[side] = dict(avg, sum=round(sum(sum(v) / len(v) for v in per.values()) / 1e3, 1))
    with open(out_split, 'w') as f:
        f.write(json.dumps(split, indent=1) + '\n')
    stats = list(csv.reader(open(stats_csv)))
    with open(out_stats, 'w', newline='') as f:
        csv.writer(f, quoting=csv.QUOTE_NONNUMERIC).writerows([stats[0]] + [r for r in stats[1:] if ours(r[0])])


if '--split' in sys.argv[1:]:
    split_trace(*sys.argv[sys.argv.index('--split') + 1:][:4])
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import demo_hot_path as demo  # noqa: E402
import sph_retina_amd as S  # noqa: E402
from fcos_bboxes_restatement import single_image  # noqa: E402
from test_bboxes_restatement import BASE_PLANAR, PANDORA  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
B, C = 8, 37
PROFILE = '--profile' in sys.argv[1:]
paths = [a for a in sys.argv[1:] if not a.startswith('--')]
out = open(paths[0], 'w') if paths else None   # the JSON lines, also printed (profiles/fcos_bboxes_bench.jsonl)


def timed(fn, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def stats(ts):
    ts = sorted(ts)
    return dict(median_us=round(statistics.median(ts), 1), p10_us=round(ts[len(ts) // 10], 1), p90_us=round(ts[len(ts) * 9 // 10], 1), steps=len(ts))


points = S.sph_fcos_points(demo.LEVEL_SHAPES, demo.FCOS_CFG['strides'], device='cuda')
n = sum(p.size(0) for p in points)
g = torch.Generator().manual_seed(2)
anchors = []
for p in points:   # the sibling's anchors: one BFoV box per point, spread over the sphere
    u = torch.rand((p.size(0), 4), generator=g)
    anchors.append(torch.stack([u[:, 0] * 360, 40 + u[:, 1] * 100, 10 + u[:, 2] * 50, 10 + u[:, 3] * 50], 1).contiguous().cuda())
point_coder = S.DistancePointSphBBoxCoder(clip_border=True, box_version=4)
delta_coder = S.DeltaXYWHSphBBoxCoder(target_means=(0.,) * 4, target_stds=(0.1, 0.1, 0.2, 0.2))
for cfg_name, cfg in (('pandora', PANDORA), ('base_planar', BASE_PLANAR)):
    for dtype in (torch.float32, torch.bfloat16):
        cls, box, ctr = demo.fcos_infer_outputs(B, C, seed=1, dtype=dtype)
        gd = torch.Generator(device='cuda').manual_seed(3)
        deltas = [(torch.randn(t.shape, generator=gd, device='cuda') * 0.5).to(dtype) for t in box]

        def batched():
            return S.sph_fcos_bboxes(cls, box, ctr, points, bbox_coder=point_coder, test_cfg=cfg, max_shape=(512, 1024))

        def per_image():
            return [single_image([t[b].float() for t in cls], [t[b].float() for t in box], [t[b].float() for t in ctr], points, point_coder, cfg, 4,
                                 'sigmoid', (512, 1024))[0] for b in range(B)]

        def sibling():
            return S.sph_test_bboxes(cls, deltas, anchors, bbox_coder=delta_coder, test_cfg=cfg, activation='sigmoid')
        if PROFILE:
            for fn in (batched, sibling):
                for _ in range(PROFILE_CALLS):
                    fn()
            torch.cuda.synchronize()
            sys.exit(0)
        for fn in (batched, sibling):
            timed(fn, WARM)
        timed(per_image, 3)
        tb, tp, ts = [], [], []
        for _ in range(STEPS // BLOCK):
            tb += timed(batched, BLOCK)
            tp += timed(per_image, max(BLOCK // 10, 1))
            ts += timed(sibling, BLOCK)
        r, rs = batched(), sibling()
        sb, ss = stats(tb), stats(ts)
        line = dict(shape=f'fcos_{n}', dtype=str(dtype).split('.')[-1], images=B, points=n, classes=C, nms_pre=1000, cfg=cfg_name, batched=sb,
                    per_image_loop=stats(tp), delta_sibling=ss, batched_minus_sibling_us=round(sb['median_us'] - ss['median_us'], 1),
                    sibling_spread_us=round(ss['p90_us'] - ss['p10_us'], 1), batched_spread_us=round(sb['p90_us'] - sb['p10_us'], 1),
                    num_dets=r.num_dets.tolist(), num_dets_sibling=rs.num_dets.tolist(), launches_batched=10)
        print(json.dumps(line), flush=True)
        if out is not None:
            out.write(json.dumps(line) + '\n')
            out.flush()
