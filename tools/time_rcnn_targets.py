"""python tools/time_rcnn_targets.py [OUT.jsonl [TRACE_DIR]] — sph_rcnn_targets at B = 8 under the reference's train_cfg.rcnn
(MaxIoUAssigner 0.5 / 0.5 / 0.5 without low-quality matches on sph2pob_standard_iou, RandomSampler num=512, pos_fraction=0.25,
add_gt_as_proposals=True, targets encoded), GT counts (64, 1, 0, 17, 64, 3, 128, 33), M = 1 000 and 2 000 padded proposals per image
in the layout of the batched inference entries (a score column, device counts between 60 % and 100 % of M):
  (i)   batched      sph_rcnn_targets: one C-ABI call, four launches, nothing read back
  (ii)  per_image    tests/rcnn_targets_restatement.rcnn_batch on the same GPU tensors: per image SphMaxIoUAssigner.assign, two nonzero,
                     two torch.randperm on the host, two unique, the index reads, bbox_coder.encode and the concatenations of
                     _get_target_single — what the parent commit offers the R-CNN stage
  (iii) kernels      the median duration of each of the four kernels from a kernel trace of `python tools/time_rcnn_targets.py --trace`
                     taken in a run of its own, whose output directory is TRACE_DIR; without it (iii) is left out.  The trace also
                     counts the launches of a call.
Device events around each step, median / p10 / p90 over settled steps; the sides alternate in blocks.  (An event bracket with a
synchronise per step adds the launch latency of the first kernel to every figure alike.)  `--trace`: 200 batched calls per shape and
nothing else, for the profiler."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import demo_hot_path as demo  # noqa: E402
import rcnn_targets_restatement as R  # noqa: E402
import sph_retina_amd as S  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
COUNTS = (64, 1, 0, 17, 64, 3, 128, 33)
SHAPES = (1000, 2000)
KERNELS = ('rcnn_pairwise_kernel', 'rcnn_candidates_kernel', 'rcnn_select_kernel', 'rcnn_compact_kernel')
CFG = R.rcnn_cfg('sph2pob_standard_iou', 4, num=512, pos_fraction=0.25)
TRACE = '--trace' in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != '--trace']
out = open(args[0], 'w') if args else None   # the JSON lines, also printed (profiles/rcnn_targets_bench.jsonl)
trace_dir = args[1] if len(args) > 1 else None


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


def kernel_medians(directory, m):
    """Per kernel the median duration (us) over the traced calls of the shape with m proposals — a call is a pairwise launch whose
    grid covers m columns and the launches up to the next pairwise launch — and the largest number of launches in one call."""
    path = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))[0]
    rows = sorted((r for r in csv.DictReader(open(path)) if 'rcnn_' in r['Kernel_Name']), key=lambda r: int(r['Dispatch_Id']))   # launch order
    calls, cur = [], None
    for r in rows:
        if KERNELS[0] in r['Kernel_Name']:
            cur = []
            calls.append((int(r['Grid_Size_X']), cur))
        if cur is not None:
            cur.append(r)
    mine = [c for gx, c in calls if gx == (m + 255) // 256 * 256]
    if not mine:
        return None
    med = {}
    for k in KERNELS:
        ts = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for c in mine for r in c if k in r['Kernel_Name']]
        med[k.replace('rcnn_', '').replace('_kernel', '') + '_us'] = round(statistics.median(ts) / 1e3, 2) if ts else None
    return med, max(len(c) for c in mine), len(mine)


gd = torch.Generator().manual_seed(0)
gts, labs = [], []
for k in COUNTS:
    u = torch.rand((k, 4), generator=gd)
    gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda())
    labs.append(torch.randint(0, 37, (k,), generator=gd).cuda())
B = len(COUNTS)
gt, lab = torch.cat(gts), torch.cat(labs)
off = torch.tensor([0] + [sum(COUNTS[:b + 1]) for b in range(B)], dtype=torch.int64).cuda()
coder = S.DeltaXYWHSphBBoxCoder(target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2))
for m in SHAPES:
    dets, num_dets = demo.synthetic_proposals(gts, m, seed=m)
    counts = num_dets.tolist()
    seed = torch.zeros((), dtype=torch.int64, device='cuda')

    def batched():
        return S.sph_rcnn_targets(dets, gt, lab, off, num_proposals=num_dets, train_cfg=CFG, num_classes=37, seed=seed, bbox_coder=coder, k_max=max(COUNTS))

    def per_image():
        return R.rcnn_batch(CFG, dets, counts, gts, labs, 37, None, coder)
    if TRACE:
        timed(batched, 200)
        continue
    t = batched()
    R.assert_equal(t, R.rcnn_batch(CFG, dets, counts, gts, labs, 37, R.ranks_of(0, B, max(COUNTS) + m).cuda(), coder), m)   # what is timed is right
    timed(batched, WARM)
    timed(per_image, 3)
    tb, tp = [], []
    for _ in range(STEPS // BLOCK):
        tb += timed(batched, BLOCK)
        tp += timed(per_image, max(BLOCK // 10, 1))
    line = dict(shape=f'B{B}_M{m}', images=B, proposals=m, num_dets=counts, num_gt=list(COUNTS), num=512, pos_fraction=0.25, backend='sph2pob_standard_iou',
                num_pos=t.num_pos.tolist(), num_neg=t.num_neg.tolist(), num_samples=float(t.num_samples), batched=stats(tb), per_image_loop=stats(tp))
    line['per_image_over_batched'] = round(line['per_image_loop']['median_us'] / line['batched']['median_us'], 1)
    if trace_dir is not None:
        k = kernel_medians(trace_dir, m)
        if k is not None:
            line.update(k[0], launches_per_call=k[1], traced_calls=k[2])
    print(json.dumps(line), flush=True)
    if out is not None:
        out.write(json.dumps(line) + '\n')
        out.flush()
