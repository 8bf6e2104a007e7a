"""python tools/bench_roi_extract.py [OUT.jsonl [TRACE_DIR]] — sph_roi_extract at the stock configuration (output 7 x 7, adaptive
sampling, aligned, strides 4 .. 32, finest_scale 56) on four levels of a 512 x 1024 image with C = 256, B = 8:
  training   512 rois per image in the reference's flat table (205 MB of output)
  inference  1 000 padded rois per image with device counts, the layout of the batched inference entries
the rois drawn like tools/demo_hot_path.synthetic_proposals.  Per shape:
  (i)   forward            one captured call, replayed: device events around each replay
  (ii)  forward_backward   the call and its backward on a fixed grad_out (zeroing launch included), captured and replayed
  (iii) kernels            the median duration of each kernel from a kernel trace of `python tools/bench_roi_extract.py --trace` taken
                           in a run of its own, whose output directory is TRACE_DIR; without it (iii) is left out
beside two references:
  floor      the time to WRITE the output's bytes at the copy rate measured here (a device-to-device copy of a buffer of the output's
             size moves twice its bytes): the feature reads are re-used across the 49 bins and the channels' planes stay in cache
  torch      the per-level torch composition of the same arithmetic on the same GPU, fp32: the box transform and the level rule as
             elementwise ops, then per level a `nonzero` (a host read), the rois' separable bilinear weight matrices (scatter_add)
             and per image two batched matmuls Wy F Wx^T — the cheapest torch formulation of RoIAlign's sums found for these shapes
             (a per-sample gather needs 49 gh gw C gathered values per roi, tens of GB at the largest grids).  It is the only baseline
             there is: the parent commit has no extractor, and neither mmcv nor torchvision exists on this stack.
What is timed is checked first: the torch composition and the extractor agree to 1e-4 of the output's scale.  Median / p10 / p90
over settled steps, the sides alternating in blocks.  `--trace`: 200 eager forward + backward calls per shape and nothing else."""
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

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 200)), 10, 25
B, C = 8, 256
CFG = dict(demo.ROI_CFG)
TRACE = '--trace' in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != '--trace']
out_file = open(args[0], 'w') if args else None
trace_dir = args[1] if len(args) > 1 else None
KERNELS = ('roi_prepare', 'roi_align_fwd', 'roi_zero', 'roi_align_bwd')


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


def proposals(m, seed):
    g = torch.Generator().manual_seed(seed)
    gts = []
    for _ in range(B):
        u = torch.rand((32, 4), generator=g)
        gts.append(torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1))
    return demo.synthetic_proposals(gts, m, seed)


def axis_weights(start, bin_size, g, bins, n):
    """(rows, bins, n) bilinear weight sums of one axis, the restatement's arithmetic in torch ops (int(g.max()) is a host read)."""
    G = max(int(g.max()), 1)
    i = torch.arange(G, device=start.device, dtype=torch.float32)
    q = torch.arange(bins, device=start.device, dtype=torch.float32)
    gf = g.clamp(min=1).float()
    y = start[:, None, None] + q[None, :, None] * bin_size[:, None, None] + (i[None, None, :] + 0.5) * bin_size[:, None, None] / gf[:, None, None]
    mask = ((i[None, None, :] < g[:, None, None]) & (y >= -1) & (y <= n)).float()
    y = y.clamp(min=0)
    lo = y.long()
    top = lo >= n - 1
    lo = torch.where(top, torch.full_like(lo, n - 1), lo).clamp(0, n - 1)
    hi = torch.where(top, lo, lo + 1).clamp(0, n - 1)
    y = torch.where(top, lo.float(), y)
    ly = y - lo.float()
    w = torch.zeros((start.size(0), bins, n), device=start.device)
    w.scatter_add_(2, lo, (1 - ly) * mask)
    w.scatter_add_(2, hi, ly * mask)
    return w


def torch_compose(feats, rois, num_rois=None):
    """The reference route in torch: flat (N, 5) rois, or padded rois with counts (flattened first, as the reference's bbox2roi does)."""
    img_h, img_w = CFG['img_shape']
    if rois.dim() == 3:
        m = rois.size(1)
        keep = (torch.arange(m, device=rois.device)[None, :] < num_rois[:, None]).reshape(-1).nonzero().squeeze(1)
        flat = torch.cat([(keep // m).float()[:, None], rois.reshape(-1, rois.size(2))[keep, :4]], dim=1)
    else:
        keep, flat = None, rois
    b = flat[:, 0].long()
    x, y, w, h = flat[:, 1] / 360 * img_w, flat[:, 2] / 180 * img_h, flat[:, 3] / 360 * img_w, flat[:, 4] / 180 * img_h
    x1, x2 = (x - w / 2).clamp(0, img_w), (x + w / 2).clamp(0, img_w)
    y1, y2 = (y - h / 2).clamp(0, img_h), (y + h / 2).clamp(0, img_h)
    lvls = torch.floor(torch.log2(torch.sqrt((x2 - x1) * (y2 - y1)) / CFG['finest_scale'] + 1e-6)).clamp(0, len(feats) - 1).long()
    ps = CFG['output_size']
    out = torch.zeros((rois.size(0) * rois.size(1) if rois.dim() == 3 else rois.size(0), feats[0].size(1), ps, ps), device=rois.device)
    for l, (f, stride) in enumerate(zip(feats, CFG['featmap_strides'])):
        inds = (lvls == l).nonzero().squeeze(1)
        if inds.numel() == 0:
            continue
        s = 1.0 / stride
        sw, sh, ew, eh = x1[inds] * s - 0.5, y1[inds] * s - 0.5, x2[inds] * s - 0.5, y2[inds] * s - 0.5
        rw, rh = ew - sw, eh - sh
        gh, gw = torch.ceil(rh / ps).long().clamp(min=0), torch.ceil(rw / ps).long().clamp(min=0)
        wy, wx = axis_weights(sh, rh / ps, gh, ps, f.size(2)), axis_weights(sw, rw / ps, gw, ps, f.size(3))
        cnt = (gh * gw).clamp(min=1).float()[:, None, None, None]
        bl = b[inds]
        for img in range(f.size(0)):
            sel = (bl == img).nonzero().squeeze(1)
            for lo in range(0, sel.numel(), 256):
                k = sel[lo:lo + 256]
                t = torch.einsum('nph,chw->ncpw', wy[k], f[img])
                rows = inds[k] if keep is None else keep[inds[k]]
                out[rows] = torch.einsum('ncpw,nqw->ncpq', t, wx[k]) / cnt[k]
    return out


def kernel_medians(directory, index):
    """Per kernel the median duration (us) of its launches in block `index` of the trace: 200 calls per shape, one launch each."""
    path = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))
    if not path:
        return None
    rows = sorted(csv.DictReader(open(path[0])), key=lambda r: int(r['Dispatch_Id']))
    med = {}
    for k in KERNELS:
        mine = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows if k + '_kernel' in r['Kernel_Name']][index * 200:(index + 1) * 200]
        if mine:
            med[k + '_us'] = round(statistics.median(mine) / 1e3, 2)
    return med


def main():
    assert torch.cuda.is_available(), 'bench_roi_extract needs an MI355X'
    feats = demo.fpn_levels(B, C, requires_grad=True)
    for index, (name, m) in enumerate((('training', 512), ('inference', 1000))):
        dets, num = proposals(m, seed=m)
        if name == 'training':   # the reference's flat table, every row live
            rois = torch.cat([torch.arange(B, device='cuda').repeat_interleave(m).float()[:, None], dets[..., :4].reshape(-1, 4)], dim=1).contiguous()
            num = None
        else:
            rois = dets
        rows = B * m
        go = torch.randn((rows, C, 7, 7), device='cuda')

        def forward():
            with torch.no_grad():
                return S.sph_roi_extract(feats, rois, num_rois=num, **CFG)

        def both():
            r = S.sph_roi_extract(feats, rois, num_rois=num, **CFG)
            return r, torch.autograd.grad(r.roi_feats, feats, go)
        if TRACE:
            timed(both, 200)
            continue
        r = forward()
        detached = [f.detach() for f in feats]
        want = torch_compose(detached, rois, num)
        err = float((r.roi_feats - want).abs().max()) / float(want.abs().max())
        assert err < 1e-4, err
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                forward()
                both()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g_fwd, g_both = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fwd):
            held = forward()
        with torch.cuda.graph(g_both):
            held_both = both()
        src, dst = torch.empty_like(r.roi_feats), torch.empty_like(r.roi_feats)
        sides = dict(forward=g_fwd.replay, forward_backward=g_both.replay, copy=lambda: dst.copy_(src),
                     torch=lambda: torch_compose(detached, rois, num))
        ts = {k: [] for k in sides}
        for k, fn in sides.items():
            timed(fn, 3 if k == 'torch' else WARM)
        for _ in range(STEPS // BLOCK):
            for k, fn in sides.items():
                ts[k] += timed(fn, max(BLOCK // 10, 1) if k == 'torch' else BLOCK)
        out_bytes = r.roi_feats.numel() * 4
        copy_us = statistics.median(ts['copy'])
        rate = 2 * out_bytes / (copy_us * 1e-6)
        line = dict(shape=f'{name}_B{B}_M{m}_C{C}', rows=rows, live_rows=int(num.sum()) if num is not None else rows, output_MB=round(out_bytes / 1e6, 1),
                    levels=torch.bincount(r.levels.long(), minlength=4).tolist(), forward=stats(ts['forward']),
                    forward_backward=stats(ts['forward_backward']), torch_composition=stats(ts['torch']), copy=stats(ts['copy']),
                    copy_rate_TBps=round(rate / 1e12, 3), write_floor_us=round(out_bytes / rate * 1e6, 1), torch_vs_extractor_rel_err=err)
        line['forward_over_floor'] = round(line['forward']['median_us'] / line['write_floor_us'], 2)
        line['torch_over_forward'] = round(line['torch_composition']['median_us'] / line['forward']['median_us'], 1)
        line['backward_share'] = round(1 - line['forward']['median_us'] / line['forward_backward']['median_us'], 3)
        if trace_dir is not None:
            k = kernel_medians(trace_dir, index)
            if k:
                line.update(k)
        del held, held_both
        print(json.dumps(line), flush=True)
        if out_file is not None:
            out_file.write(json.dumps(line) + '\n')
            out_file.flush()


if __name__ == '__main__':
    main()
