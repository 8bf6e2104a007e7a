"""python tools/time_test_bboxes.py [OUT.jsonl] — sph_test_bboxes at 98 208 anchors, C = 37, B = 8, nms_pre = 1000 for the four variants, against the per-image composition
(tests/test_bboxes_restatement.single_image on each image: what the parent commit offers for these calculators).
Device events around each step, median / p10 / p90 over settled steps; the two alternate in blocks."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402

import demo_hot_path as demo  # noqa: E402
import sph_retina_amd as S  # noqa: E402
from test_bboxes_restatement import BASE_PLANAR, BASE_PLANAR_TAN, INDOOR360, PANDORA, single_image  # noqa: E402

STEPS, WARM, BLOCK = int(os.environ.get('STEPS', 300)), 30, 50
B = 8
out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None   # the JSON lines, also printed (profiles/test_bboxes_timing.jsonl)


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


for name, cfg, dim in (('unbiased', PANDORA, 5), ('unbiased_bfov', PANDORA, 4), ('naive', INDOOR360, 4), ('planar_sph2pix', BASE_PLANAR, 4),
                       ('planar_sph2tan', BASE_PLANAR_TAN, 4), ('sph2pob_efficient', dict(PANDORA, iou_calculator='sph2pob_efficient'), 4)):
    anchors = demo.retina_level_anchors()
    if dim == 5:
        g = torch.Generator().manual_seed(7)
        anchors = [torch.cat([a, (torch.rand((a.size(0), 1), generator=g) * 120 - 60).cuda()], 1).contiguous() for a in anchors]
    cls, box = demo.head_outputs(B, 37, dim=dim, seed=dim)
    coder = (S.DeltaXYWHSphBBoxCoder(target_means=(0.,) * 4, target_stds=(0.1, 0.1, 0.2, 0.2)) if dim == 4 else
             S.DeltaXYWHASphBBoxCoder(target_means=(0.,) * 5, target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)))

    def batched():
        return S.sph_test_bboxes(cls, box, anchors, bbox_coder=coder, test_cfg=cfg, box_version=dim, activation='none')

    def per_image():
        return [single_image([c[b] for c in cls], [p[b] for p in box], anchors, coder, cfg, dim)[0] for b in range(B)]
    timed(batched, WARM)
    timed(per_image, 5)
    tb, tp = [], []
    for _ in range(STEPS // BLOCK):
        tb += timed(batched, BLOCK)
        tp += timed(per_image, max(BLOCK // 5, 1))
    r = batched()
    line = dict(variant=name, box_dim=dim, images=B, anchors=sum(a.size(0) for a in anchors), classes=37, nms_pre=1000,
                batched=stats(tb), per_image_loop=stats(tp), num_dets=r.num_dets.tolist(), launches_batched=10)
    print(json.dumps(line), flush=True)
    if out is not None:
        out.write(json.dumps(line) + '\n')
        out.flush()
