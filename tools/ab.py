#!/usr/bin/env python3
"""A/B timing of several builds / load-time settings of libsph2pob_hip.so on ONE box in ONE process.

Boxes differ by a few percent and so do the first thousand launches of a process, so arms are interleaved in rounds and
the median over rounds is what counts.  Two steps, because hipcc time on the GPU box is GPU budget:

  build (here, no GPU):   python tools/ab.py build base fence=-DSPH_ASSIGN_FENCE,-DFOO=1 ...
                          -> build/ab/<label>.so   (label alone = the shipped flags; the tree's .so files travel with gpurun)
  run   (GPU box):        python tools/ab.py run --workload assign --tag r05_assign base fence other=base:SPH2POB_PW_ROWS=12
                          an arm is <label>[=<built label>][:ENV=val[,ENV=val]]  (load-time knobs are read when the copy is loaded)
                          -> one line per arm and size on stdout and, with --tag, in gpurun_out/<tag>.log (copy to profiles/)

Workloads (all through the C ABI, buffers allocated once, HIP events around `--launches` back-to-back calls):
  aligned   sph2pob_iou_aligned_f32, --pairs N[,N..] --dim 4|5 --variant standard|efficient|legacy [--nearby SIGMA] [--reference-order]
  pairwise  sph2pob_iou_pairwise_f32 on configs[3] (64 GT x the ERP anchor grids)
  assign    pairwise + sph2pob_assign_f32 (the matrix route) on the same
  fused     sph2pob_iou_assign_f32 (no matrix) on the same
  anchor_targets  sph2pob_anchor_targets_f32 (the batched route): 8 images x 64 GT x the 98 208 anchors of the 512 x 1024 ERP
  loss      sph2pob_loss_fwd_grad_f32 + final sum + grad_scale, 1 M nearby RBFoV pairs, CIoU (configs[2])
  nms       sph2pob_nms_segmented_f32 on 5 000 sorted boxes x 37 classes and on one class of 5 000
  bnms      sph2pob_batched_nms_f32 (unsorted input, no host work) on the same two scenes
  head_losses  sph2pob_{focal,bbox,delta}_loss_sum_f32, each timed on its own, with gradients: 8 images x the 5 NCHW levels of the
            512 x 1024 ERP (98 208 anchors), 37 classes, dim 4, CIoU closed-form / L1, ~1 % live rows, a device avg_factor; then
            sph2pob_gauss_bbox_loss_sum_f32 (kld) on the same, or on an arm without it the composition through that library's
            decode, Gaussian loss and decode-adjoint entries; then the
            same on bf16 levels, forward + first backward with g = 1 and g = 0.5: sph2pob_*_sum_h16 where the arm's library has
            them, the cast route (.float(), the _f32 entry, the stash scaling, .to(bfloat16)) where it has not (the parent build)
  test_bboxes_h16  sph2pob_test_bboxes on bf16 levels at that shape (PANDORA's test_cfg): the _h16 entry, or .float() + the _f32 entry
  bboxes    one call per batched inference entry under PANDORA's test_cfg, fp32, BFoV, 8 images x 37 classes, the inputs of the
            tools/time_*_bboxes.py scripts: sph2pob_test_bboxes_f32 and sph2pob_softmax_bboxes_f32 on the 98 208 anchors,
            sph2pob_fcos_bboxes_f32 on the 10 912 points, sph2pob_rcnn_bboxes_f32 on 1 000 padded rois per image
  adjoint   sph2pob_transform_bwd_f32 / _general_f32, every instantiated (variant, dim) x edge x angle x jitter, --pairs N
Every arm's outputs are compared with the first arm's (bit equality is reported, not assumed).
"""
import argparse
import ctypes
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AB_DIR = os.path.join(ROOT, 'build', 'ab')


def build(specs):
    from sph_retina_amd import _lib
    os.makedirs(AB_DIR, exist_ok=True)
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    procs = []
    for spec in specs:
        label, _, flags = spec.partition('=')
        out = os.path.join(AB_DIR, label + '.so')
        cmd = [hipcc] + _lib.HIPCC_FLAGS + [f for f in flags.split(',') if f] + ['-o', out] + \
            [os.path.join(_lib.CSRC, s) for s in _lib.SOURCES]
        procs.append((label, out, subprocess.Popen(cmd, cwd=_lib.CSRC)))
        if len(procs) % 4 == 0:   # four compilers at a time (8 cores, ~1 GB each)
            for _l, _o, p in procs[-4:]:
                p.wait()
    for label, out, p in procs:
        assert p.wait() == 0, label
        print('built', os.path.relpath(out, ROOT))


def load_arms(specs, tmp):
    from sph_retina_amd import _lib
    arms = []
    for k, spec in enumerate(specs):
        head, _, envs = spec.partition(':')
        label, _, built = head.partition('=')
        path = os.path.join(AB_DIR, (built or label) + '.so')
        if not os.path.exists(path) and (built or label) == 'shipped':
            path = _lib.LIB_PATH
        saved = {}
        for kv in filter(None, envs.split(',')):
            key, val = kv.split('=')
            saved[key] = os.environ.get(key)
            os.environ[key] = val
        copy = os.path.join(tmp, f'arm{k}.so')
        shutil.copy(path, copy)
        lib = ctypes.CDLL(copy)
        for key, old in saved.items():
            if old is None:
                del os.environ[key]
            else:
                os.environ[key] = old
        for name, argtypes in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.argtypes = argtypes
                fn.restype = _lib._RESTYPES.get(name, ctypes.c_int)
        arms.append((label, lib))
    return arms


def _gt64(torch, k=64):
    g = torch.Generator().manual_seed(0)
    u = torch.rand((k, 4), generator=g)
    return torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 85, 5 + u[:, 3] * 85], 1).cuda()


def workloads(args, torch, G):
    """Yields (title, make(lib) -> (launch, outputs))."""
    st = G.raw_stream_of(torch.device('cuda', 0))
    if args.workload == 'aligned':
        from bench import make_boxes
        variant = {'standard': 0, 'efficient': 1, 'legacy': 2, 'sph_iou': 3, 'fov_iou': 4, 'unbiased': 5, 'naive': 6}[args.variant] | (0x100 if args.reference_order else 0)
        for n in [int(x) for x in args.pairs.split(',')]:
            if args.dim == 4:
                b1, b2 = make_boxes(n, 0, 'cuda'), make_boxes(n, 1, 'cuda')
            else:
                g = torch.Generator().manual_seed(0)
                u = torch.rand((2, n, 5), generator=g)
                mk = lambda v: torch.stack([v[:, 0] * 360, v[:, 1] * 180, v[:, 2] * 99 + 1, v[:, 3] * 99 + 1, v[:, 4] * 180 - 90], 1)  # noqa: E731
                b1, b2 = mk(u[0]).cuda(), mk(u[1]).cuda()
            if args.nearby > 0:
                g = torch.Generator().manual_seed(5)
                b2 = b1 + (torch.randn(b1.shape, generator=g) * args.nearby).cuda()
                b2[:, 0] %= 360
                b2[:, 1:4] = b2[:, 1:4].clamp(1, 179)
                b2 = b2.contiguous()

            def make(lib, b1=b1, b2=b2, n=n):
                out = torch.empty(n, device='cuda')
                return (lambda: lib.sph2pob_iou_aligned_f32(G.ptr(b1), G.ptr(b2), G.ptr(out), n, args.dim, variant, 0, 0, 0, st)), [out]
            yield f'aligned {args.variant} dim {args.dim} pairs {n}', make
    elif args.workload in ('pairwise', 'assign', 'fused'):
        from tools.bench_configs import retina_anchors
        for grid in ((512, 1024), (1024, 2048)):
            anchors, gt = retina_anchors(*grid), _gt64(torch)
            k, n = 64, anchors.size(0)
            labels = (torch.arange(k) % 37).cuda()

            def make(lib, anchors=anchors, gt=gt, k=k, n=n, labels=labels):
                mo, gi, lab = torch.empty(n, device='cuda'), torch.empty(n, dtype=torch.int64, device='cuda'), torch.empty(n, dtype=torch.int64, device='cuda')
                amo, gm, gam = torch.empty(n, dtype=torch.int64, device='cuda'), torch.empty(k, device='cuda'), torch.empty(k, dtype=torch.int64, device='cuda')
                if args.workload == 'fused':
                    ws = torch.empty(lib.sph2pob_iou_assign_workspace_bytes(k, n) // 8, dtype=torch.int64, device='cuda')
                    state = torch.zeros(lib.sph2pob_iou_assign_state_bytes(k, n) // 8, dtype=torch.int64, device='cuda')

                    def launch():
                        return lib.sph2pob_iou_assign_f32(G.ptr(gt), k, G.ptr(anchors), n, 4, 0, 0, None, None, 0.5, 0.0, 0.4, 0.0, 1, 1,
                                                          G.ptr(labels), G.ptr(mo), G.ptr(amo), G.ptr(gm), G.ptr(gam), G.ptr(gi), G.ptr(lab),
                                                          G.ptr(ws), G.ptr(state), st)
                    return launch, [mo, amo, gm, gam, gi, lab]
                ov = torch.empty((k, n), device='cuda')
                ws = torch.empty(lib.sph2pob_assign_workspace_bytes(k, n) // 8, dtype=torch.int64, device='cuda')

                def launch():
                    rc = lib.sph2pob_iou_pairwise_f32(G.ptr(gt), k, G.ptr(anchors), n, G.ptr(ov), 4, 0, 0, 0, 0, st)
                    if args.workload == 'assign':
                        rc |= lib.sph2pob_assign_f32(G.ptr(ov), k, n, 0.5, 0.0, 0.4, 0.0, 1, 1, G.ptr(labels), G.ptr(mo), G.ptr(amo), G.ptr(gm),
                                                     G.ptr(gam), G.ptr(gi), G.ptr(lab), G.ptr(ws), st)
                    return rc
                return launch, ([ov] if args.workload == 'pairwise' else [ov, mo, amo, gm, gam, gi, lab])
            yield f'{args.workload} 64 x {n}', make
    elif args.workload == 'anchor_targets':
        from tools.bench_configs import retina_anchors
        anchors, B, km = retina_anchors(512, 1024), 8, 64
        n, K = anchors.size(0), B * km
        gt, labels = _gt64(torch, K), (torch.arange(K) % 37).cuda()
        off = (torch.arange(B + 1) * km).cuda()

        def make(lib):
            i64, f32 = dict(dtype=torch.int64, device='cuda'), dict(dtype=torch.float32, device='cuda')
            o = [torch.empty((B, n), **i64), torch.empty((B, n), **f32), torch.empty((B, n), **i64), torch.empty((B, n), **i64),
                 torch.empty((B, n), **f32), torch.empty((B, n, 4), **f32), torch.empty((B, n, 4), **f32), torch.empty(B, **i64),
                 torch.empty(B, **i64), torch.empty(1, **f32)]
            ws = torch.empty(lib.sph2pob_anchor_targets_workspace_bytes(B, K, km, n) // 8, **i64)
            state = torch.zeros(lib.sph2pob_anchor_targets_state_bytes(B, km, n) // 8, **i64)
            return (lambda: lib.sph2pob_anchor_targets_f32(G.ptr(anchors), n, G.ptr(gt), G.ptr(labels), G.ptr(off), B, K, km, 4, 0, 0, 0.5, 0.0, 0.4, 0.0,
                                                           1, 1, 37, -1.0, 0, None, None, *[G.ptr(t) for t in o], G.ptr(ws), G.ptr(state), st)), o
        yield f'anchor_targets {B} x {km} x {n}', make
    elif args.workload == 'loss':
      for n in ([int(v) for v in args.pairs.split(',')] if args.pairs != '1000000' else [1_000_000]):
          g = torch.Generator().manual_seed(2)
          u = torch.rand((n, 5), generator=g)
          tgt = torch.stack([u[:, 0] * 360, u[:, 1] * 180, u[:, 2] * 99 + 1, u[:, 3] * 99 + 1, u[:, 4] * 180 - 90], 1)
          pred = tgt + torch.randn((n, 5), generator=g) * torch.tensor([8., 8., 6., 6., 10.])
          pred[:, 0] %= 360
          pred[:, 1] = pred[:, 1].clamp(0.5, 179.5)
          pred[:, 2:4] = pred[:, 2:4].clamp(1, 170)
          pred[:, 4] = pred[:, 4].clamp(-89, 89)
          pred, tgt = pred.cuda().contiguous(), tgt.cuda().contiguous()
          for mode_name, mode in (('ciou', 3), ('iou', 0)):
              def make(lib, mode=mode):
                  gp, out = torch.empty((n, 5), device='cuda'), torch.empty(1, device='cuda')
                  ws = torch.empty(lib.sph2pob_loss_sum_workspace_floats(n) + 1024, device='cuda')
                  one = torch.ones(1, device='cuda')

                  def launch():
                      rc = lib.sph2pob_loss_fwd_grad_f32(G.ptr(pred), G.ptr(tgt), None, 0, 1.0 / n, None, G.ptr(out), G.ptr(ws), G.ptr(gp), None, n, 5,
                                                         mode, 1e-6, st)
                      return rc | lib.sph2pob_loss_grad_scale_f32(G.ptr(gp), G.ptr(one), 0, G.ptr(gp), n, 5, st)
                  return launch, [out, gp]
              yield f'loss {mode_name} fwd+grad {n} RBFoV', make
    elif args.workload in ('nms', 'bnms'):
        import numpy as np
        from tools.bench_configs import boxes
        k = 5000
        rng = np.random.default_rng(4)
        centres = boxes(300, 8, alpha=(5, 60)).cpu().numpy()
        b = centres[rng.integers(0, 300, k)] + rng.standard_normal((k, 4)).astype(np.float32) * 2.0
        b[:, 0] %= 360
        b[:, 1] = b[:, 1].clip(1, 179)
        b[:, 2:] = b[:, 2:].clip(2, 120)
        scores = torch.rand(k, generator=torch.Generator().manual_seed(1))
        for title, cls in (('5000 x 37 classes', torch.randint(0, 37, (k,), generator=torch.Generator().manual_seed(2))),
                           ('5000 x 1 class', torch.zeros(k, dtype=torch.int64))):
            order = torch.argsort(cls.double() * 2 - scores.double(), stable=True)
            bs, cs = torch.from_numpy(b)[order].cuda().contiguous(), cls[order].cuda().contiguous()
            seg = int(torch.bincount(cls).max())

            if args.workload == 'bnms':
                ub, us, uc = torch.from_numpy(b).cuda().contiguous(), scores.cuda(), (cls.cuda() if title.endswith('classes') else None)
                mx = 100 if uc is not None else k

                def make(lib, ub=ub, us=us, uc=uc, mx=mx):
                    ws = torch.empty(lib.sph2pob_batched_nms_workspace_bytes(k, 4), dtype=torch.uint8, device='cuda')
                    ko, do, stt = torch.zeros(mx, dtype=torch.int64, device='cuda'), torch.zeros((mx, 5), device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
                    return (lambda: lib.sph2pob_batched_nms_f32(G.ptr(ub), G.ptr(us), G.ptr(uc), k, 4, 1, 0.5, mx, G.ptr(ws), G.ptr(ko), G.ptr(do),
                                                                G.ptr(stt), st)), [ko, do, stt]
                yield f'bnms {title}', make
                continue

            def make(lib, bs=bs, cs=cs, seg=seg):
                keep = torch.empty(k, dtype=torch.uint8, device='cuda')
                ws = torch.empty(lib.sph2pob_nms_segmented_workspace_bytes(k, seg) // 8 + 8, dtype=torch.int64, device='cuda')
                return (lambda: lib.sph2pob_nms_segmented_f32(G.ptr(bs), G.ptr(cs), k, 4, 1, 0.5, seg, G.ptr(ws), G.ptr(keep), st)), [keep]
            yield f'nms {title}', make
    elif args.workload == 'head_losses':
        import math
        from tools import demo_hot_path as D
        images, classes, levels = 8, 37, len(D.LEVEL_SHAPES)
        anchors = torch.cat(D.retina_level_anchors())
        n = anchors.size(0)
        g = torch.Generator().manual_seed(6)
        live = torch.rand((images, n), generator=g) < 0.01     # the positives of bench_configs.bbox_loss are of this order
        weights = live[:, :, None].float().expand(images, n, 4).contiguous().cuda()
        boxes = anchors.cpu()[None] + torch.randn((images, n, 4), generator=g) * torch.tensor([2., 2., 1., 1.])
        boxes[..., 2:] = boxes[..., 2:].clamp(1, 179)
        boxes, deltas_t = boxes.contiguous().cuda(), (torch.randn((images, n, 4), generator=g) * 0.1).cuda()
        labels = torch.where(live, torch.randint(0, classes, (images, n), generator=g), torch.tensor(classes)).cuda()
        avg = live.sum().float().reshape(1).cuda()
        cls = [(torch.randn((images, 9 * classes, h, w), generator=g) * 2 - 4).cuda() for h, w in D.LEVEL_SHAPES]
        box = [(torch.randn((images, 9 * 4, h, w), generator=g) * 0.05).cuda() for h, w in D.LEVEL_SHAPES]
        ptrs, i64s, f4 = ctypes.c_void_p * levels, ctypes.c_int64 * levels, ctypes.c_float * 4
        ns, hws = i64s(*[9 * h * w for h, w in D.LEVEL_SHAPES]), i64s(*[h * w for h, w in D.LEVEL_SHAPES])
        means, stds, max_ratio = f4(0, 0, 0, 0), f4(1, 1, 1, 1), abs(math.log(16 / 1000))

        def entry(name, xs, last, call):
            def make(lib):
                grads = [torch.empty_like(x) for x in xs]
                out = torch.empty(1, device='cuda')
                ws = torch.empty(getattr(lib, f'sph2pob_{name}_workspace_bytes')(ns, hws, levels, images, last), dtype=torch.uint8, device='cuda')
                xp, gp = ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in grads])
                return (lambda: call(lib, xp, gp, G.ptr(out), G.ptr(ws))), [out] + grads
            return f'head_losses {name}_sum fwd+grad {images} x {n}', make
        yield entry('focal_loss', cls, classes, lambda lib, xp, gp, out, ws: lib.sph2pob_focal_loss_sum_f32(
            xp, gp, ns, hws, levels, images, classes, G.ptr(labels), None, 0, 2.0, 0.25, 1.0, G.ptr(avg), out, ws, st))
        yield entry('bbox_loss', box, 4, lambda lib, xp, gp, out, ws: lib.sph2pob_bbox_loss_sum_f32(
            xp, gp, ns, hws, levels, images, 4, G.ptr(anchors), G.ptr(boxes), G.ptr(weights), 4, means, stds,
            max_ratio, 1, 32.0, 3, 1e-6, 1.0, G.ptr(avg), out, ws, st))
        yield entry('delta_loss', box, 4, lambda lib, xp, gp, out, ws: lib.sph2pob_delta_loss_sum_f32(
            xp, gp, ns, hws, levels, images, 4, G.ptr(deltas_t), G.ptr(weights), 4, 0.0, 1.0, G.ptr(avg), out, ws, st))

        # The Gaussian regression loss (kld, log1p, tau 1).  An arm whose library has sph2pob_gauss_bbox_loss_sum_f32 takes it; an arm
        # without it (the parent build) takes the composition a head ran there, through that library's own entries: permute /
        # reshape / cat of the levels, sph2pob_coder_decode_f32 over all B n rows, sph2pob_gauss_loss_fwd_grad_f32 over all B n
        # rows, the division by the device avg_factor, sph2pob_coder_decode_bwd_f32, split + permute back.  Its figure therefore
        # includes the torch copies a head makes around the entries (five permute copies in, two scalings, five permute copies
        # out: thirteen torch launches beside the three entries); the B n x 4 buffers are allocated once, outside the timing.  Outputs: the
        # loss and the NCHW gradients (the two routes scale in a different order: equal values, not equal bits).
        gauss = (1, 1, 1.0, 1.0, 1, 0.0, 0.0)   # SPH2POB_GAUSS_KLD, log1p, tau, alpha, sqrt, beta, eps
        rois = anchors.repeat(images, 1).contiguous()
        total = images * n
        eps32 = float(torch.finfo(torch.float32).eps)

        def gauss_entry():
            def make(lib):
                fused = getattr(lib, 'sph2pob_gauss_bbox_loss_sum_f32', None)
                grads = [torch.empty_like(x) for x in box]
                out = torch.empty(1, device='cuda')
                if fused is not None:
                    ws = torch.empty(lib.sph2pob_gauss_bbox_loss_workspace_bytes(ns, hws, levels, images, 4), dtype=torch.uint8, device='cuda')
                    xp, gp = ptrs(*[G.ptr(x) for x in box]), ptrs(*[G.ptr(v) for v in grads])
                    return (lambda: fused(xp, gp, ns, hws, levels, images, 4, G.ptr(anchors), G.ptr(boxes), G.ptr(weights), 4, means, stds,
                                          max_ratio, 1, 32.0, *gauss, 1.0, G.ptr(avg), G.ptr(out), G.ptr(ws), st)), [out] + grads
                ws = torch.empty(lib.sph2pob_loss_sum_workspace_floats(total), device='cuda')
                flat, dec, gbox, gflat = (torch.empty((total, 4), device='cuda') for _ in range(4))   # allocated once, outside the timing
                sizes = [9 * h * w for h, w in D.LEVEL_SHAPES]

                def launch():
                    for fl, x in zip(flat.view(images, n, 4).split(sizes, 1), box):   # the permute + cat copies of the head
                        fl.copy_(x.permute(0, 2, 3, 1).reshape(images, -1, 4))
                    rc = lib.sph2pob_coder_decode_f32(G.ptr(rois), G.ptr(flat), means, stds, G.ptr(dec), total, 1, 4, max_ratio, 1, 32.0, st)
                    rc |= lib.sph2pob_gauss_loss_fwd_grad_f32(G.ptr(dec), G.ptr(boxes), G.ptr(weights), 4, 1.0, None, G.ptr(out), G.ptr(ws),
                                                              G.ptr(gbox), None, total, 4, *gauss, st)
                    k = 1.0 / (avg + eps32)
                    out.mul_(k)
                    gbox.mul_(k)
                    rc |= lib.sph2pob_coder_decode_bwd_f32(G.ptr(rois), G.ptr(flat), G.ptr(gbox), means, stds, G.ptr(gflat), total, 1, 4, max_ratio,
                                                           1, 32.0, st)
                    for gl, v, (h, w) in zip(gflat.view(images, n, 4).split(sizes, 1), grads, D.LEVEL_SHAPES):
                        v.copy_(gl.reshape(images, h, w, 9 * 4).permute(0, 3, 1, 2))
                    return rc
                return launch, [out] + grads
            return f'head_losses gauss_bbox_loss_sum kld fwd+grad {images} x {n}', make
        yield gauss_entry()

        # bf16 levels, forward + first backward with an upstream gradient g.  An arm whose library has the _h16 entries takes the
        # native route (the entry with a bf16 stash, then the gradient-only call with grad_out = g, skip_if_one = 1); an arm
        # without them (the parent build) takes what a bf16 caller got there: .float() of the levels, the _f32 entry with
        # gradients, the stash scaling, .to(bfloat16) of the gradients.  The outputs compared are the loss and the bf16 gradients.
        bf = torch.bfloat16
        cls16, box16 = [x.to(bf) for x in cls], [x.to(bf) for x in box]

        def entry16(name, xs, last, args, gval):
            def make(lib):
                out = torch.empty(1, device='cuda')
                ws = torch.empty(getattr(lib, f'sph2pob_{name}_workspace_bytes')(ns, hws, levels, images, last), dtype=torch.uint8, device='cuda')
                g = torch.full((1,), gval, device='cuda')
                h16 = getattr(lib, f'sph2pob_{name}_sum_h16', None)
                held = {}
                if h16 is not None:
                    grads = [torch.empty_like(x) for x in xs]
                    xp, gp = ptrs(*[G.ptr(x) for x in xs]), ptrs(*[G.ptr(v) for v in grads])

                    def launch():
                        rc = h16(xp, gp, ns, hws, levels, images, last, *args, G.ptr(out), G.ptr(ws), None, 0, 2, st)
                        return rc | h16(xp, gp, ns, hws, levels, images, last, *args, None, None, G.ptr(g), 1, 2, st)
                    return launch, [out] + grads
                f32 = getattr(lib, f'sph2pob_{name}_sum_f32')
                grads = [torch.empty_like(x) for x in xs]   # the bf16 gradients the caller ends up with

                def launch():
                    fs = [x.float() for x in xs]
                    stash = [torch.empty_like(f) for f in fs]
                    rc = f32(ptrs(*[G.ptr(f) for f in fs]), ptrs(*[G.ptr(v) for v in stash]), ns, hws, levels, images, last, *args, G.ptr(out),
                             G.ptr(ws), st)
                    for v, o in zip(stash, grads):
                        rc |= lib.sph2pob_focal_loss_grad_scale_f32(G.ptr(v), G.ptr(g), G.ptr(v), v.numel(), st)
                        o.copy_(v)   # the narrowing cast
                    held['last'] = (fs, stash)
                    return rc
                return launch, [out] + grads
            return f'head_losses bf16 {name} fwd+bwd g={gval} {images} x {n}', make
        for gval in (1.0, 0.5):
            yield entry16('focal_loss', cls16, classes, (G.ptr(labels), None, 0, 2.0, 0.25, 1.0, G.ptr(avg)), gval)
            yield entry16('bbox_loss', box16, 4, (G.ptr(anchors), G.ptr(boxes), G.ptr(weights), 4, means, stds, max_ratio, 1, 32.0, 3, 1e-6,
                                                  1.0, G.ptr(avg)), gval)
            yield entry16('delta_loss', box16, 4, (G.ptr(deltas_t), G.ptr(weights), 4, 0.0, 1.0, G.ptr(avg)), gval)
    elif args.workload == 'test_bboxes_h16':
        # sph2pob_test_bboxes on bf16 levels (PANDORA's test_cfg, 8 images x the 5 NCHW levels, 37 classes): the _h16 entry where the
        # arm's library has it, the parent's route (.float() of every level, then the _f32 entry) where it has not
        import math
        from tools import demo_hot_path as D
        images, classes, levels = 8, 37, len(D.LEVEL_SHAPES)
        anchors = D.retina_level_anchors()
        cls, box = D.head_outputs(images, classes)
        cls, box = [x.to(torch.bfloat16) for x in cls], [x.to(torch.bfloat16) for x in box]
        ptrs, i64s, f4 = ctypes.c_void_p * levels, ctypes.c_int64 * levels, ctypes.c_float * 4
        ns, hws = i64s(*[9 * h * w for h, w in D.LEVEL_SHAPES]), i64s(*[h * w for h, w in D.LEVEL_SHAPES])
        means, stds, max_ratio = f4(0, 0, 0, 0), f4(0.1, 0.1, 0.2, 0.2), abs(math.log(16 / 1000))
        ap = ptrs(*[G.ptr(a) for a in anchors])

        def make(lib):
            f32, i64 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int64, device='cuda')
            o = [torch.empty((images, 100, 5), **f32), torch.empty((images, 100), **i64), torch.empty((images, 100), **i64), torch.empty((images,), **i64)]
            ws = torch.empty(lib.sph2pob_get_bboxes_workspace_bytes(ns, levels, images, classes, 4, 1000), dtype=torch.uint8, device='cuda')
            mid = (ns, hws, levels, images, classes, 4, 0, 0.05, 1000, means, stds, max_ratio, 1, 32.0, 5, 0, 0.5, 100, *[G.ptr(t) for t in o], G.ptr(ws))
            h16 = getattr(lib, 'sph2pob_test_bboxes_h16', None)
            if h16 is not None:
                cp, bp = ptrs(*[G.ptr(x) for x in cls]), ptrs(*[G.ptr(x) for x in box])
                return (lambda: h16(cp, bp, ap, *mid, 2, st)), o
            held = {}

            def launch():
                cf, bf32 = [x.float() for x in cls], [x.float() for x in box]
                held['last'] = (cf, bf32)
                return lib.sph2pob_test_bboxes_f32(ptrs(*[G.ptr(x) for x in cf]), ptrs(*[G.ptr(x) for x in bf32]), ap, *mid, st)
            return launch, o
        yield f'test_bboxes bf16 unbiased {images} x {sum(a.size(0) for a in anchors)}', make
    elif args.workload == 'bboxes':
        import math
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import rcnn_bboxes_restatement as R
        import sph_retina_amd as S
        from tools import demo_hot_path as D
        images, classes, levels = 8, 37, len(D.LEVEL_SHAPES)
        ptrs, i64s, f4 = ctypes.c_void_p * levels, ctypes.c_int64 * levels, ctypes.c_float * 4
        f32, i64 = dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.int64, device='cuda')
        coder = (f4(0, 0, 0, 0), f4(0.1, 0.1, 0.2, 0.2), abs(math.log(16 / 1000)), 1, 32.0)   # means, stds, max_ratio, coder_flags, ctr_clamp
        nms = (5, 0, 0.5, 100)                                                                # unbiased, per class, iou_threshold, max_per_img

        def outputs(extra=0):
            return [torch.empty((images, 100, 5), **f32), torch.empty((images, 100), **i64), torch.empty((images, 100), **i64)] + \
                [torch.empty((images,), **i64) for _ in range(1 + extra)]

        def workspace(shared, need):
            """One workspace per entry for all arms (they run one after the other on one stream): byte-identical selection kernels
            differed by up to 10 us between arms that had a workspace each, more than any difference between the builds."""
            ws = shared.setdefault('ws', torch.empty(need, dtype=torch.uint8, device='cuda'))
            assert ws.numel() == need
            return ws

        def table(tensors):
            return ptrs(*[G.ptr(t) for t in tensors])

        def dense(name, symbol, ws_symbol, heads, priors, per_position, head_args):
            """A dense head's entry: `heads` are its level tensor lists in the order of the entry's pointer tables."""
            ns, hws = i64s(*[per_position * h * w for h, w in D.LEVEL_SHAPES]), i64s(*[h * w for h, w in D.LEVEL_SHAPES])
            tables = [table(x) for x in heads[:2]] + [table(priors)] + [table(x) for x in heads[2:]]

            shared = {}

            def make(lib, held=(heads, priors)):   # (the tables hold addresses only: the tensors live as long as the launch does)
                o = outputs()
                ws = workspace(shared, getattr(lib, ws_symbol)(ns, levels, images, classes, 4, 1000))
                fn = getattr(lib, symbol)
                return (lambda: fn(*tables, ns, hws, levels, images, classes, 4, *head_args, *nms, *[G.ptr(t) for t in o], G.ptr(ws), st)), o
            return f'bboxes {name} unbiased {images} x {sum(p.size(0) for p in priors)}', make

        anchors = D.retina_level_anchors()
        yield dense('test_bboxes_f32', 'sph2pob_test_bboxes_f32', 'sph2pob_get_bboxes_workspace_bytes', D.head_outputs(images, classes, dim=4, seed=4),
                    anchors, 9, (0, 0.05, 1000, *coder))
        yield dense('softmax_bboxes_f32', 'sph2pob_softmax_bboxes_f32', 'sph2pob_softmax_bboxes_workspace_bytes',
                    D.softmax_head_outputs(images, classes, seed=1), anchors, 9, (0.05, 1000, *coder))
        points = S.sph_fcos_points(D.LEVEL_SHAPES, D.FCOS_CFG['strides'], device='cuda')
        yield dense('fcos_bboxes_f32', 'sph2pob_fcos_bboxes_f32', 'sph2pob_get_bboxes_workspace_bytes', D.fcos_infer_outputs(images, classes, seed=1),
                    points, 1, (1, 0.05, 1000, 512, 1024, 512.0, 1024.0))

        m, cap = 1000, 16384   # the default capacity of sph_rcnn_bboxes at score_thr 0.05: min(M * 20, sph2pob_batched_nms_max_boxes())
        g = torch.Generator().manual_seed(m)
        counts = tuple(int(m * (0.6 + 0.4 * float(torch.rand((), generator=g)))) for _ in range(images))
        rois, num, logits, box = R.scene(4, 5, 'per_class', 'cuda', seed=m, counts=counts, m=m, num_classes=classes)

        shared = {}

        def make(lib):
            o = outputs(extra=1)   # num_valid
            ws = workspace(shared, lib.sph2pob_rcnn_bboxes_workspace_bytes(images, m, classes + 1, 4, cap))
            return (lambda: lib.sph2pob_rcnn_bboxes_f32(G.ptr(rois), G.ptr(num), G.ptr(logits), G.ptr(box), images, m, rois.size(2), classes + 1, 4, 0,
                                                        0.05, cap, *coder, *nms, *[G.ptr(t) for t in o], G.ptr(ws), st)), o
        yield f'bboxes rcnn_bboxes_f32 unbiased {images} x {m} rois', make
    elif args.workload == 'adjoint':
        n = int(args.pairs.split(',')[0])
        g = torch.Generator().manual_seed(7)
        u = torch.rand((n, 5), generator=g)
        b1 = torch.stack([u[:, 0] * 360, u[:, 1] * 180, u[:, 2] * 99 + 1, u[:, 3] * 99 + 1, u[:, 4] * 180 - 90], 1)
        b2 = b1 + torch.randn((n, 5), generator=g) * torch.tensor([8., 8., 6., 6., 10.])   # a third nearby, a third equal, the rest unrelated
        b2[n // 3:2 * n // 3] = b1[n // 3:2 * n // 3]
        b2[2 * n // 3:] = b1[torch.randperm(n, generator=g)[2 * n // 3:]]
        g1, g2 = torch.randn((n, 5), generator=g).cuda(), torch.randn((n, 5), generator=g).cuda()
        for general, variant, dim in [(gen, v, d) for gen in (0, 1) for v, d in ((0, 4), (0, 5), (1, 4), (1, 5), (2, 4)) if gen or v < 2]:
            x, y = b1[:, :dim].contiguous().cuda(), b2[:, :dim].contiguous().cuda()
            for edge, angle, jitter in [(e, a, j) for e in (0, 1, 2) for a in ((0, 1) if general else (0,)) for j in (0, 1)]:
                def make(lib, x=x, y=y, variant=variant, dim=dim, edge=edge, angle=angle, jitter=jitter, general=general):
                    o = [torch.empty((n, dim), device='cuda'), torch.empty((n, dim), device='cuda')]
                    p = [G.ptr(t) for t in (x, y, g1, g2, *o)]
                    if general:
                        return (lambda: lib.sph2pob_transform_bwd_general_f32(*p, n, dim, variant, edge, angle, jitter, st)), o
                    return (lambda: lib.sph2pob_transform_bwd_f32(*p, n, dim, variant, edge, jitter, st)), o
                yield f'adjoint {"dual" if general else "closed"} variant {variant} dim {dim} edge {edge} angle {angle} jitter {jitter} pairs {n}', make
    else:
        raise SystemExit('unknown workload ' + args.workload)


def run(args):
    import torch
    from sph_retina_amd import _torch_glue as G
    tmp = tempfile.mkdtemp(prefix='ab_')
    arms = load_arms(args.arms, tmp)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for title, make in workloads(args, torch, G):
        made = [make(lib) for _label, lib in arms]
        for (label, _), (launch, _o) in zip(arms, made):
            rc = launch()
            assert rc == 0, (label, rc)
        torch.cuda.synchronize()
        for (label, _), (_l, outs) in zip(arms[1:], made[1:]):
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, made[0][1]))
            say(f'{title}: {label} vs {arms[0][0]}: outputs {"bit-equal" if same else "DIFFER"}')
        for i in range(args.settle):
            made[i % len(arms)][0]()
        torch.cuda.synchronize()
        times = [[] for _ in arms]
        for _r in range(args.rounds):
            for k, (launch, _o) in enumerate(made):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.launches * 1e3)
        for (label, _), t in zip(arms, times):
            say(f'{title}: {label:24s} median {statistics.median(t):8.3f} us  min {min(t):8.3f}  max-min {max(t) - min(t):7.3f}  '
                f'all {" ".join("%.2f" % x for x in t)}')
    shutil.rmtree(tmp, ignore_errors=True)
    if args.tag:
        os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
        with open(os.path.join(ROOT, 'gpurun_out', args.tag + '.log'), 'w') as f:
            f.write('# python tools/ab.py ' + ' '.join(sys.argv[1:]) + '\n' + '\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    b = sub.add_parser('build')
    b.add_argument('specs', nargs='+')
    r = sub.add_parser('run')
    r.add_argument('--workload', default='aligned')
    r.add_argument('--pairs', default='1000000')
    r.add_argument('--dim', type=int, default=4)
    r.add_argument('--variant', default='standard')
    r.add_argument('--nearby', type=float, default=0.0)
    r.add_argument('--reference-order', action='store_true')
    r.add_argument('--rounds', type=int, default=5)
    r.add_argument('--launches', type=int, default=300)
    r.add_argument('--settle', type=int, default=2000)
    r.add_argument('--tag', default='')
    r.add_argument('arms', nargs='+')
    args = ap.parse_args()
    if args.cmd == 'build':
        build(args.specs)
    else:
        run(args)


if __name__ == '__main__':
    main()
