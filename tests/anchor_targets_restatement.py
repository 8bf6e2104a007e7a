"""Shared by tests/test_anchor_targets_host.py and tests/test_gpu_anchor_targets.py: the target construction of mmdet's
AnchorHead._get_targets_single (anchor_head.py:254-285, PseudoSampler, every anchor valid) written out in torch from the
semantics table of include/sph2pob_hip.h, applied to ONE image's AssignResult, and the comparison of a batched result with
per-image `SphMaxIoUAssigner.assign` calls + that transcription.  Everything is compared for exact equality."""
import torch


def targets_single(anchors, gt, gt_labels, assign_result, num_classes, pos_weight=-1, coder=None):
    """-> labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg for one image."""
    n = anchors.size(0)
    gt_inds = assign_result.gt_inds
    pos_inds = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1)      # PseudoSampler
    neg_inds = torch.nonzero(gt_inds == 0, as_tuple=False).squeeze(-1)
    bbox_targets = torch.zeros_like(anchors)
    bbox_weights = torch.zeros_like(anchors)
    labels = anchors.new_full((n,), num_classes, dtype=torch.long)
    label_weights = anchors.new_zeros(n, dtype=torch.float)
    if len(pos_inds) > 0:
        pos_gt = gt[gt_inds[pos_inds] - 1]
        bbox_targets[pos_inds] = pos_gt if coder is None else coder.encode(anchors[pos_inds], pos_gt)
        bbox_weights[pos_inds] = 1.0
        labels[pos_inds] = 0 if gt_labels is None else gt_labels[gt_inds[pos_inds] - 1]
        label_weights[pos_inds] = 1.0 if pos_weight <= 0 else pos_weight
    if len(neg_inds) > 0:
        label_weights[neg_inds] = 1.0
    return labels, label_weights, bbox_targets, bbox_weights, len(pos_inds), len(neg_inds)


def check_batch(out, assigner, anchors, gt_list, labels_list, num_classes, pos_weight=-1, coder=None):
    """Every field of the batched result `out` against per-image assign + targets_single; returns the per-image results."""
    B = len(gt_list)
    assert out.gt_inds.shape == out.labels.shape == out.label_weights.shape == out.max_overlaps.shape == (B, anchors.size(0))
    assert out.bbox_targets.shape == out.bbox_weights.shape == (B,) + tuple(anchors.shape)
    singles, total = [], 0
    for b, gt in enumerate(gt_list):
        gl = None if labels_list is None else labels_list[b]
        res = assigner.assign(anchors, gt, gt_labels=gl)
        singles.append(res)
        assert torch.equal(out.gt_inds[b], res.gt_inds), b
        assert torch.equal(out.max_overlaps[b], res.max_overlaps), b
        if gl is not None:
            assert torch.equal(out.assigned_labels[b], res.labels), b
        else:
            assert out.assigned_labels is None and res.labels is None
        lab, lw, bt, bw, npos, nneg = targets_single(anchors, gt, gl, res, num_classes, pos_weight, coder)
        assert torch.equal(out.labels[b], lab), b
        assert torch.equal(out.label_weights[b], lw), b
        assert torch.equal(out.bbox_targets[b], bt), b
        assert torch.equal(out.bbox_weights[b], bw), b
        assert int(out.num_pos[b]) == npos and int(out.num_neg[b]) == nneg, (b, int(out.num_pos[b]), npos, int(out.num_neg[b]), nneg)
        total += max(npos, 1)
    assert float(out.avg_factor) == float(total)
    return singles
