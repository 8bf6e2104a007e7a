"""python tools/time_rcnn_bboxes.py [OUT.jsonl [TRACE_DIR]] — sph_rcnn_bboxes at B = 8, C = 37, BFoV, under the reference's
test_cfg.rcnn (score_thr 0.05, iou_threshold 0.5, max_per_img 100) with PANDORA's `unbiased_iou` and with the base configuration's
`planar`, M = 1 000 and 2 000 padded rois per image in the layout of the batched inference entries (a score column, device counts
between 60 % and 100 % of M), per-class deltas, the default capacity:
  (i)   batched      sph_rcnn_bboxes: one C-ABI call, eleven launches, nothing read back
  (ii)  per_image    tests/rcnn_bboxes_restatement.single_image on the same GPU tensors, image after image: sph_softmax_scores,
                     bbox_coder.decode of all M C boxes and multiclass_nms with its nonzero and the NMS's host reads — what the
                     parent commit offers the R-CNN stage at inference
  (iii) kernels      the median duration of each kernel of a call from a kernel trace of `python tools/time_rcnn_bboxes.py --trace`
                     taken in a run of its own, whose output directory is TRACE_DIR; without it (iii) is left out.  The trace also
                     counts the launches of a call.
Device events around each step, median / p10 / p90 over settled steps; the sides alternate in blocks.  (An event bracket with a
synchronise per step adds the launch latency of the first kernel to every figure alike.)  `--trace`: 200 batched calls per shape
and configuration and nothing else, for the profiler."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import rcnn_bboxes_restatement as R  # noqa: E402
import sph_retina_amd as S  # noqa: E402
from test_bboxes_restatement import BASE_PLANAR, PANDORA  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
B, C = 8, 37
SHAPES = (1000, 2000)
CFGS = (('unbiased_iou', R.rcnn_cfg(PANDORA)), ('planar', R.rcnn_cfg(BASE_PLANAR)))
FIRST = 'rcnn_prob_kernel'   # the first launch of a call
TRACE = '--trace' in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != '--trace']
out = open(args[0], 'w') if args else None   # the JSON lines, also printed (profiles/rcnn_bboxes_bench.jsonl)
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


def short(name):
    """'void (anonymous namespace)::topk_hist_kernel<float>(...)' -> 'topk_hist'"""
    name = name.replace('(anonymous namespace)::', '').split('<')[0].split('(')[0]   # up to the template or argument list
    return name.split()[-1].split('::')[-1].replace('_kernel', '')


def kernel_medians(directory, index):
    """The traced calls come in blocks of 200 per (shape, configuration), in the order of the loops below.  Per kernel name the
    median of the summed duration (us) of its launches in one call of block `index`; the launches of a call."""
    path = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Dispatch_Id']))   # launch order
    calls, cur = [], None
    for r in rows:
        if FIRST in r['Kernel_Name']:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append(r)
    mine = calls[index * 200:(index + 1) * 200]
    if not mine:
        return None
    launches = statistics.median(len(c) for c in mine)
    mine = [c for c in mine if len(c) == launches]   # (the last call of the trace may have other work behind it)
    med = {}
    for k in sorted({short(r['Kernel_Name']) for r in mine[0]}):
        per_call = [sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in c if short(r['Kernel_Name']) == k) for c in mine]
        med[k + '_us'] = round(statistics.median(per_call) / 1e3, 2)
    return med, int(launches), len(mine)


coder = R.coder_for(4)
index = 0
for m in SHAPES:
    g = torch.Generator().manual_seed(m)
    counts = tuple(int(m * (0.6 + 0.4 * float(torch.rand((), generator=g)))) for _ in range(B))
    rois, num, logits, box = R.scene(4, 5, 'per_class', 'cuda', seed=m, counts=counts, m=m, num_classes=C)
    for name, cfg in CFGS:
        def batched():
            return S.sph_rcnn_bboxes(rois, logits, box, num_rois=num, bbox_coder=coder, test_cfg=cfg, num_classes=C)

        def per_image():
            return [R.single_image(rois[b], counts[b], logits[b], box[b], coder, cfg, 4) for b in range(B)]
        if TRACE:
            timed(batched, 200)
            continue
        r = batched()
        kept, valid = R.check_batch(r, rois, counts, logits, box, coder, cfg, 4)   # what is timed is right
        timed(batched, WARM)
        timed(per_image, 3)
        tb, tp = [], []
        for _ in range(STEPS // BLOCK):
            tb += timed(batched, BLOCK)
            tp += timed(per_image, max(BLOCK // 10, 1))
        line = dict(shape=f'B{B}_M{m}_C{C}', images=B, rois=m, num_rois=list(counts), iou_calculator=name, max_candidates=r.max_candidates,
                    num_valid=valid, num_dets=kept, batched=stats(tb), per_image_loop=stats(tp))
        line['per_image_over_batched'] = round(line['per_image_loop']['median_us'] / line['batched']['median_us'], 1)
        if trace_dir is not None:
            k = kernel_medians(trace_dir, index)
            if k is not None:
                line.update(k[0], launches_per_call=k[1], traced_calls=k[2])
        index += 1
        print(json.dumps(line), flush=True)
        if out is not None:
            out.write(json.dumps(line) + '\n')
            out.flush()
