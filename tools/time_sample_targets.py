"""python tools/time_sample_targets.py [OUT.jsonl [TRACE_DIR]] — sph_sample_targets at B = 8 under an RPN sampler (num=256,
pos_fraction=0.5) on the targets sph_train_targets gives under the RPN assigner (0.7 / 0.3 / 0.3), at the RetinaNet shape (98 208
anchors) and at SSD300's 8 732 anchors:
  (i)   inplace       sph_sample_targets(inplace=True): what sph_rpn_targets runs
  (ii)  out_of_place  sph_sample_targets into new tensors
  (iii) per_image     tests/sample_targets_restatement.sample_batch on the GPU tensors: per image nonzero, torch.randperm on the host,
                      unique, twice, then the index writes of _get_targets_single — what the parent commit offers a sampling head
  (iv)  apply         the bytes the apply pass must move in place (per row: assigned_gt_inds 8 + rank 4 read, flag 1 written; per row
                      that leaves the sample: label 8 + weight 4 + 2 box rows written) over its kernel time, as a fraction of the
                      6.3 TB/s a float4 copy reaches on this chip.  Kernel times are not visible to events around a call: they come
                      from a kernel trace of `python tools/time_sample_targets.py --trace` taken in a run of its own, whose output
                      directory is TRACE_DIR; without it (iv) is left out.
  (v)   caller_ranks  (i) with the caller's own ranks (the generator's, precomputed): the select pass without the Philox evaluation, so
                      (i) - (v) is what evaluating the ranks once costs the one workgroup of an (image, side) — and what every further
                      pass would cost again if the ranks were recomputed instead of written to the workspace and read back
Device events around each step, median / p10 / p90 over settled steps; the sides alternate in blocks.  (An event bracket with a
synchronise per step adds the launch latency of the first kernel to every figure alike; the differences are not affected.)
`--trace`: 200 in-place calls per shape and nothing else, for the profiler."""
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
import sample_targets_restatement as R  # noqa: E402
import sph_retina_amd as S  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
COUNTS = (64, 1, 0, 17, 64, 3, 128, 33)
HBM_TBPS = 6.3
SAMPLER = dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False)
TRAIN_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1,
                               iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4)),
                 allowed_border=-1, pos_weight=-1, debug=False)
TRACE = '--trace' in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != '--trace']
out = open(args[0], 'w') if args else None   # the JSON lines, also printed (profiles/sample_targets_bench.jsonl)
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


def kernel_medians(directory, grid_x_apply):
    """Median durations (us) of the two kernels out of a kernel-trace CSV: the apply launches with this grid, and the select launches
    that precede them (grid 1024 B x 2)."""
    path = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))[0]
    rows = [r for r in csv.DictReader(open(path)) if 'sample_' in r['Kernel_Name']]
    apply_t, select_t = [], []
    for prev, r in zip(rows, rows[1:]):
        if 'sample_apply_kernel' in r['Kernel_Name'] and int(r['Grid_Size_X']) == grid_x_apply and 'sample_select_kernel' in prev['Kernel_Name']:
            apply_t.append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
            select_t.append(int(prev['End_Timestamp']) - int(prev['Start_Timestamp']))
    return (statistics.median(apply_t) / 1e3, statistics.median(select_t) / 1e3, len(apply_t)) if apply_t else None


gd = torch.Generator().manual_seed(0)
gts = []
for k in COUNTS:
    u = torch.rand((k, 4), generator=gd)
    gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda())
B = len(COUNTS)
for name, anchors in (('retina_98208', demo.retina_anchors()), ('ssd300_8732', torch.cat(demo.ssd300_level_anchors()))):
    n = anchors.size(0)
    base = S.sph_train_targets(anchors, gts, train_cfg=TRAIN_CFG, num_classes=1)
    work = R.clone(base)
    seed = torch.zeros((), dtype=torch.int64, device='cuda')

    def inplace():
        # (rows that left the sample of the previous step read as they were written then: the selection reads assigned_gt_inds only,
        # and the apply pass writes the same bytes whatever the row held)
        return S.sph_sample_targets(work, sampler=SAMPLER, num_classes=1, seed=seed, inplace=True)

    def out_of_place():
        return S.sph_sample_targets(base, sampler=SAMPLER, num_classes=1, seed=seed)

    def per_image():
        return R.sample_batch(base, 1, 256, 0.5, -1)
    own = R.ranks_of(0, B, n)
    own = torch.where(own >= 1 << 31, own - (1 << 32), own).to(torch.int32).cuda()   # the 32 bits the kernels read

    def caller_ranks():
        return S.sph_sample_targets(work, sampler=SAMPLER, num_classes=1, seed=0, ranks=own, inplace=True)
    if TRACE:
        timed(inplace, 200)
        continue
    assert torch.equal(caller_ranks().sample_flags, inplace().sample_flags)
    for fn in (inplace, out_of_place, caller_ranks):
        timed(fn, WARM)
    timed(per_image, 3)
    ti, to, tp, tr = [], [], [], []
    for _ in range(STEPS // BLOCK):
        ti += timed(inplace, BLOCK)
        to += timed(out_of_place, BLOCK)
        tp += timed(per_image, max(BLOCK // 10, 1))
        tr += timed(caller_ranks, BLOCK)
    r = out_of_place()
    kept = int((r.sample_flags != 0).sum()) + int((base.gt_inds < 0).sum())
    moved = B * n * 13 + (B * n - kept) * (12 + 2 * 4 * 4)
    line = dict(shape=name, images=B, anchors=n, num=256, pos_fraction=0.5, positives=base.num_pos.tolist(), ignored=int((base.gt_inds < 0).sum()),
                num_pos=r.num_pos.tolist(), num_neg=r.num_neg.tolist(), avg_factor=float(r.avg_factor), inplace=stats(ti), out_of_place=stats(to),
                per_image_loop=stats(tp), caller_ranks=stats(tr), apply_bytes_inplace=moved, launches=2)
    if trace_dir is not None:
        per_image_blocks = (n // 4 + 255) // 256 if n % 4 == 0 else (n + 255) // 256
        k = kernel_medians(trace_dir, per_image_blocks * 256)
        if k is not None:
            line.update(apply_kernel_us=round(k[0], 2), select_kernel_us=round(k[1], 2), traced_calls=k[2], apply_tbps=round(moved / k[0] / 1e6, 3),
                        apply_fraction_of_hbm=round(moved / k[0] / 1e6 / HBM_TBPS, 3))
    print(json.dumps(line), flush=True)
    if out is not None:
        out.write(json.dumps(line) + '\n')
        out.flush()
