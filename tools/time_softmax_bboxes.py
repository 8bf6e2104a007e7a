"""python tools/time_softmax_bboxes.py [OUT.jsonl] — sph_softmax_bboxes at B = 8, K = 38 (C = 37), nms_pre = 1000 under the PANDORA
configuration, at the RetinaNet shape (98 208 anchors) and at SSD300's 8 732 anchors, for fp32 and float16 levels:
  (i)   batched      sph_softmax_bboxes
  (ii)  per_image    torch softmax(-1)[..., :-1] on every level, then tests/test_bboxes_restatement.single_image on each image: what
                     the parent commit offers a softmax head
  (iii) sigmoid      sph_test_bboxes(activation='sigmoid') on C channels at the same shape: the sibling; (i) - (iii) is what the
                     softmax stage costs
  (iv)  scores       sph_softmax_scores alone, with the bytes it must move (the logits once at their dtype + C fp32 per anchor
                     written) over its time, as a fraction of the 6.3 TB/s a float4 copy reaches on this chip
Device events around each step, median / p10 / p90 over settled steps; the sides alternate in blocks.  (An event bracket with a
synchronise per step adds the launch latency of the first kernel to every figure alike; the differences are not affected.)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import demo_hot_path as demo  # noqa: E402
import sph_retina_amd as S  # noqa: E402
from test_bboxes_restatement import PANDORA, single_image  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
B, C = 8, 37
HBM_TBPS = 6.3
out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None   # the JSON lines, also printed (profiles/softmax_bboxes_bench.jsonl)


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


SHAPES = (('retina_98208', demo.LEVEL_SHAPES, 9, demo.retina_level_anchors),
          ('ssd300_8732', demo.SSD300_SHAPES, demo.SSD300_ANCHORS, demo.ssd300_level_anchors))
coder = S.DeltaXYWHSphBBoxCoder(target_means=(0.,) * 4, target_stds=(0.1, 0.1, 0.2, 0.2))
for name, shapes, per, make_anchors in SHAPES:
    for dtype in (torch.float32, torch.float16):
        anchors = make_anchors()
        n = sum(a.size(0) for a in anchors)
        cls, box = demo.softmax_head_outputs(B, C, seed=1, shapes=shapes, anchors_per_position=per, dtype=dtype)
        # the sibling's logits: logit(p) of the softmax head's own probabilities — the same scores, so the same selection load
        sig = [(p.double().log() - torch.log1p(-p.double())).clamp(-30, 30).to(dtype).contiguous() for p in S.sph_softmax_scores(cls, num_classes=C)]

        def batched():
            return S.sph_softmax_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=PANDORA)

        def per_image():
            probs = [torch.softmax(t.float().reshape(B, -1, C + 1, t.size(2), t.size(3)), 2)[:, :, :C].reshape(B, -1, t.size(2), t.size(3)) for t in cls]
            return [single_image([p[b] for p in probs], [d[b].float() for d in box], anchors, coder, PANDORA, 4)[0] for b in range(B)]

        def sigmoid():
            return S.sph_test_bboxes(sig, box, anchors, bbox_coder=coder, test_cfg=PANDORA, activation='sigmoid')

        def scores():
            return S.sph_softmax_scores(cls, num_classes=C)
        for fn in (batched, sigmoid, scores):
            timed(fn, WARM)
        timed(per_image, 3)
        tb, tp, ts, tc = [], [], [], []
        for _ in range(STEPS // BLOCK):
            tb += timed(batched, BLOCK)
            tp += timed(per_image, max(BLOCK // 10, 1))
            ts += timed(sigmoid, BLOCK)
            tc += timed(scores, BLOCK)
        r, rs = batched(), sigmoid()
        moved = B * n * ((C + 1) * cls[0].element_size() + C * 4)
        sc = stats(tc)
        line = dict(shape=name, dtype=str(dtype).split('.')[-1], images=B, anchors=n, channels=C + 1, nms_pre=1000, cfg='pandora',
                    batched=stats(tb), per_image_loop=stats(tp), sigmoid_sibling=stats(ts), scores_only=sc, scores_bytes=moved,
                    scores_tbps=round(moved / sc['median_us'] / 1e6, 3), scores_fraction_of_hbm=round(moved / sc['median_us'] / 1e6 / HBM_TBPS, 3),
                    prob_traffic_bytes=3 * B * n * C * 4, num_dets=r.num_dets.tolist(), num_dets_sigmoid=rs.num_dets.tolist(), launches_batched=11)
        print(json.dumps(line), flush=True)
        if out is not None:
            out.write(json.dumps(line) + '\n')
            out.flush()
