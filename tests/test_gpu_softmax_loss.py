"""GPU: the fused softmax cross-entropy kernels, plain and mined, against the f64 truth (the checks of softmax_restatement.py on
the device), against their host twins, and the sync-free step sph_anchor_targets -> sph_softmax_loss(neg_pos_ratio=3,
avg_factor=device scalar) -> backward captured into a graph.

Device and host twins run one row function; their expf / log1p come from different math libraries, so the two are held to the
element bound against each other rather than bit for bit (measured maxima: DESIGN.md §4.11)."""
import pytest
import torch

import softmax_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('k', (2, 6, 38))
def test_grid_accuracy_and_better_than_the_composition(S, k):
    R.check_grid(S, 'cuda', k)


def test_tails_are_finite_signed_and_close(S):
    R.check_tails(S, 'cuda')


def test_scene_mining_layouts_and_divisors(S):
    R.check_scene(S, 'cuda')


def test_scene_k38(S):
    R.check_k38(S, 'cuda')


def test_several_workgroups_scene(S):
    R.check_scene(S, 'cuda', levels=R.BIG_LEVELS, seed=R.BIG_SEED, need_cut=3)


def test_ties_take_the_lowest_rows(S):
    R.check_ties(S, 'cuda')


def test_ties_over_several_chunks_of_the_walk(S):
    R.check_ties_over_several_chunks(S, 'cuda')


def test_ties_in_the_padded_tail_all_taken_and_all_but_one(S):
    R.check_ties_in_the_padded_tail(S, 'cuda')


def test_nan_loss_is_mined_first_and_reaches_the_sum(S):
    R.check_nan_loss_is_mined_first(S, 'cuda')


def test_plain_mode_function_and_module(S):
    R.check_plain_and_module(S, 'cuda')


@pytest.mark.parametrize('levels,seed', ((R.SCENE_LEVELS, R.SCENE_SEED), (R.BIG_LEVELS, R.BIG_SEED)))
def test_two_calls_give_the_same_bits(S, levels, seed):
    R.check_determinism(S, 'cuda', levels, seed)


def test_unaligned_base_takes_the_scalar_kind(S):
    """A level whose base pointer is one float off 16-byte alignment (a view into a buffer): the same bits as the aligned call."""
    scores, labels, weights = R.scene(R.SCENE_LEVELS[:1])
    s = scores[0].cuda()
    buf = torch.empty(s.numel() + 1, device='cuda')
    off = buf[1:].view(s.shape)
    off.copy_(s)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    a_in, b_in = s.clone().requires_grad_(True), off.detach().requires_grad_(True)
    a = S.sph_softmax_loss([a_in], labels.cuda(), weights.cuda(), neg_pos_ratio=R.RATIO, avg_factor=4.0)
    b = S.sph_softmax_loss([b_in], labels.cuda(), weights.cuda(), neg_pos_ratio=R.RATIO, avg_factor=4.0)
    assert float(a) == float(b)
    assert torch.equal(torch.autograd.grad(a, a_in)[0], torch.autograd.grad(b, b_in)[0])


def test_device_equals_host_twin(S):
    figures = {}
    for k in (2, 6, 38):
        x, labels = R.grid_inputs(k)
        dev = R.flat_loss_and_grads(S, x, labels, 'cuda')
        host = R.flat_loss_and_grads(S, x, labels, 'cpu')
        for name, d, h in zip(('loss', 'grad_flat', 'grad_fused'), dev, host):
            figures[f'grid K={k} {name}'] = (R.rel_err(d, h.double())[0], bool(torch.equal(d.cpu(), h)))
    for levels, seed in ((R.SCENE_LEVELS, R.SCENE_SEED), (R.BIG_LEVELS, R.BIG_SEED)):
        scores, lab, w = R.scene(levels, seed=seed)
        outs = []
        for device in ('cuda', 'cpu'):
            ins = [s.clone().to(device).requires_grad_(True) for s in scores]
            loss, rows = R.run_levels(S, ins, lab.to(device), w.to(device), neg_pos_ratio=R.RATIO, avg_factor=5.0)
            outs.append((loss.detach().cpu(), rows.cpu()))
        assert torch.equal(R.support(outs[0][1]), R.support(outs[1][1])), 'device and host twin mine the same rows'
        figures[f'scene n={lab.size(1)} grad'] = (R.rel_err(outs[0][1], outs[1][1].double())[0], bool(torch.equal(outs[0][1], outs[1][1])))
        figures[f'scene n={lab.size(1)} loss'] = (R.rel_err(outs[0][0], outs[1][0].double())[0], bool(torch.equal(outs[0][0], outs[1][0])))
    for name, (r, same) in figures.items():
        print(f'softmax device vs host {name}: max rel {r:.3e} bit-equal {same}')
    for name, (r, same) in figures.items():
        assert r <= R.REL_GRID, (name, r)


def test_targets_loss_backward_capture_into_a_graph(S):
    """sph_anchor_targets -> sph_softmax_loss(neg_pos_ratio=3, avg_factor=t.avg_factor) -> backward on the small scene: one stream,
    no parallel branches, nothing read back; two replays with changed logits equal the eager step bit for bit."""
    C = R.K - 1
    scores, _, _ = R.scene()
    n = sum(s.size(1) // R.K * s.size(2) * s.size(3) for s in scores)
    g = torch.Generator().manual_seed(3)
    u = torch.rand((n, 4), generator=g)
    anchors = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 60, 5 + u[:, 3] * 60], 1).cuda()
    counts = [4, 0, 3, 2]
    k = sum(counts)
    pick = torch.randint(0, n, (k,), generator=g)
    gt = (anchors[pick.cuda()] + 0.5).contiguous()
    gt_labels = torch.randint(0, C, (k,), generator=g).cuda()
    offsets = torch.tensor([0, 4, 4, 7, 9], dtype=torch.int64).cuda()
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4))
    ins = [s.cuda().requires_grad_(True) for s in scores]

    def step():
        t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4)
        loss = S.sph_softmax_loss(ins, t.labels, t.label_weights, neg_pos_ratio=R.RATIO, avg_factor=t.avg_factor)
        return (loss,) + torch.autograd.grad(loss, ins) + (t.num_pos,)

    def load(seed):
        with torch.no_grad():
            for x, s in zip(ins, R.scene(seed=seed)[0]):
                x.copy_(s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (21, 22):
        load(seed)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in captured]
        want = step()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert torch.isfinite(got[0]) and float(got[0]) > 0 and int(got[-1].sum()) > 0 and bool((got[1] != 0).any())
        rows = R.to_rows(got[1:-1]).reshape(-1, R.K)
        assert 0 < int(R.support(rows).sum()) < rows.size(0), 'some rows are mined, most are not'
