"""python tools/bench_rcnn_loss.py [OUT.jsonl [TRACE_DIR]] — the box loss of the R-CNN head at the stock shape: B = 8 images, 512
sampled rows each (S = 4 096), C = 37 classes, dim = 4 — a (4 096, 148) head output, 2.4 MB of gradient — on the table
`sph_rcnn_targets` makes of tools/demo_hot_path's two-stage scene, with `avg_factor=t.num_samples`.  Forward + backward to
`bbox_pred`, captured into a graph and replayed between device events, for both loss families:
  fused        `sph_rcnn_bbox_loss` (sph2pob_rcnn_delta_loss_sum_f32 / sph2pob_rcnn_bbox_loss_sum_f32)
  composition  what the step ran before: `rcnn_bbox_pred` (torch.gather) -> L1Loss, and -> bbox_coder.decode -> Sph2PobIoULoss, the
               gather's backward (a zero tensor and a scatter) included
in the same run, the sides alternating in blocks: median / p10 / p90 over settled replays.  What is timed is checked first: the
two routes agree (the gradient to 4 ulp per element, the loss to 1e-5).  Then the demo's whole two-stage training step
(`run_batch(rcnn_cfg=..., roi_extract=True)`: features -> RoI extractor -> two Linear heads -> losses -> all gradients) with and
without `fused_losses=True`, as graph replays timed on the host over 50 replays.
`--trace`: 200 eager forward + backward calls of the fused route per family and nothing else — for a kernel trace taken in a run of
its own, whose output directory is TRACE_DIR: the median duration of each kernel is then added to the lines."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import demo_hot_path as demo  # noqa: E402
import sph_retina_amd as S  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 400)), 20, 50
C, NUM = 37, 512
TRACE = '--trace' in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != '--trace']
out_file = open(args[0], 'w') if args else None
trace_dir = args[1] if len(args) > 1 else None
RCNN_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1,
                              iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4)),
                sampler=dict(type='RandomSampler', num=NUM, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1, debug=False)
FAMILIES = (('l1_encoded', False, 'rcnn_delta_loss'), ('iou_decoded', True, 'rcnn_bbox_loss'))


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
    return dict(median_us=round(statistics.median(ts), 2), p10_us=round(ts[len(ts) // 10], 2), p90_us=round(ts[len(ts) * 9 // 10], 2), steps=len(ts))


def kernel_medians(directory, index, kernel):
    """The median duration (us) of the family's loss kernel and of the final pass in block `index` of the trace (200 calls each)."""
    path = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))
    if not path:
        return None
    rows = sorted(csv.DictReader(open(path[0])), key=lambda r: int(r['Dispatch_Id']))
    med = {}
    for key, name, block in ((kernel + '_kernel_us', kernel + '_kernel', 0), ('head_final_kernel_us', 'head_final_kernel', index)):
        mine = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows if name in r['Kernel_Name']][block * 200:(block + 1) * 200]
        if mine:
            med[key] = round(statistics.median(mine) / 1e3, 2)
    return med


def routes(t, coder, bbox_pred, decoded):
    loss_l1, loss_iou = S.L1Loss(loss_weight=1.0), S.Sph2PobIoULoss(mode='iou', loss_weight=1.0)
    cfg = dict(type='Sph2PobIoULoss', mode='iou') if decoded else dict(type='L1Loss')

    def fused():
        loss = S.sph_rcnn_bbox_loss(bbox_pred, t.labels, t.bbox_targets, t.bbox_weights, num_classes=C, loss_bbox=cfg,
                                    rois=t.rois if decoded else None, bbox_coder=coder if decoded else None, avg_factor=t.num_samples)
        return loss.detach(), torch.autograd.grad(loss, bbox_pred)[0]

    def composition():
        picked = S.rcnn_bbox_pred(bbox_pred, t.labels, C, 4, False)
        if decoded:
            loss = loss_iou(coder.decode(t.rois[:, 1:].contiguous(), picked), t.bbox_targets, t.bbox_weights, avg_factor=t.num_samples)
        else:
            loss = loss_l1(picked, t.bbox_targets, t.bbox_weights, avg_factor=t.num_samples)
        return loss.detach(), torch.autograd.grad(loss, bbox_pred)[0]
    return fused, composition


def main():
    assert torch.cuda.is_available(), 'bench_rcnn_loss needs an MI355X'
    for index, (name, decoded, kernel) in enumerate(FAMILIES):
        info, d = demo.run_batch(num_classes=C, rcnn_cfg=RCNN_CFG, rcnn_decoded=decoded, reps=1)
        t, coder, bbox_pred = d['targets'], d['coder'], d['bbox_pred']
        fused, composition = routes(t, coder, bbox_pred, decoded)
        if TRACE:
            timed(fused, 200)
            continue
        (lf, gf), (lc, gc) = fused(), composition()
        eps = float(torch.finfo(torch.float32).eps)
        assert torch.equal(gf == 0, gc == 0) and bool(((gf - gc).abs() <= 4 * eps * gc.abs()).all()) and bool((gf != 0).any())
        assert abs(float(lf) - float(lc)) <= 1e-5 * abs(float(lc)), (float(lf), float(lc))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fused()
                composition()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g_fused, g_comp = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fused):
            held = fused()
        with torch.cuda.graph(g_comp):
            held_comp = composition()
        sides = dict(fused=g_fused.replay, composition=g_comp.replay)
        ts = {k: [] for k in sides}
        for fn in sides.values():
            timed(fn, WARM)
        for _ in range(STEPS // BLOCK):
            for k, fn in sides.items():
                ts[k] += timed(fn, BLOCK)
        line = dict(shape=f'{name}_B8_num{NUM}_C{C}_dim4', rows=int(bbox_pred.size(0)), positives=int(sum(info['num_pos'])), gradient_MB=round(bbox_pred.numel() * 4 / 1e6, 2),
                    loss=float(lf), fused=stats(ts['fused']), composition=stats(ts['composition']))
        line['composition_over_fused'] = round(line['composition']['median_us'] / line['fused']['median_us'], 2)
        del held, held_comp
        step = {}
        for flag in (False, True):
            step['fused_losses' if flag else 'composition'] = round(demo.run_batch(num_classes=C, rcnn_cfg=RCNN_CFG, rcnn_decoded=decoded, roi_extract=True,
                                                                                   fused_losses=flag, reps=50)[0]['graph_replay_ms'], 3)
        line['two_stage_step_ms'] = step
        if trace_dir is not None:
            k = kernel_medians(trace_dir, index, kernel)
            if k:
                line.update(k)
        print(json.dumps(line), flush=True)
        if out_file is not None:
            out_file.write(json.dumps(line) + '\n')
            out_file.flush()


if __name__ == '__main__':
    main()
