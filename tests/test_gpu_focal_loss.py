"""GPU: the fused sigmoid focal loss kernels against the f64 restatement (the checks of focal_restatement.py on the device),
against their host twins, and the sync-free step sph_anchor_targets -> sph_focal_loss(avg_factor=device scalar) -> backward
captured into a graph.

Device and host twins run one element function; their expf / log1pf come from different math libraries, so the two are held to
the element bound against each other rather than bit for bit (measured maxima: DESIGN.md, the sigmoid focal loss subsection)."""
import pytest
import torch

import focal_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    assert torch.cuda.is_available()
    return sph_retina_amd


@pytest.mark.parametrize('gamma,alpha', R.GAMMA_ALPHA)
def test_grid_accuracy_and_better_than_the_composition(S, gamma, alpha):
    R.check_grid(S, 'cuda', gamma, alpha)


@pytest.mark.parametrize('gamma,alpha', R.GAMMA_ALPHA)
def test_tails_are_finite_signed_and_close(S, gamma, alpha):
    R.check_tails(S, 'cuda', gamma, alpha)


def test_scene_layouts_weights_reductions_and_divisors(S):
    R.check_scene(S, 'cuda')


def test_scene_general_gamma(S):
    R.check_scene(S, 'cuda', gamma=1.5, alpha=0.4)


def test_multi_workgroup_scene_matches_f64(S):
    R.check_scene(S, 'cuda', levels=R.BIG_LEVELS)


def test_edge_cases(S):
    R.check_edges(S, 'cuda')


@pytest.mark.parametrize('levels', (R.SCENE_LEVELS, R.BIG_LEVELS))
def test_two_calls_give_the_same_bits(S, levels):
    R.check_determinism(S, 'cuda', levels)


def test_unaligned_base_takes_the_scalar_path(S):
    """A level whose base pointer is not 16-byte aligned (a view one float into a buffer): the same bits as the aligned call."""
    scores, labels, w_row, _ = R.scene(R.SCENE_LEVELS[:1])
    s = scores[0].cuda()
    buf = torch.empty(s.numel() + 1, device='cuda')
    off = buf[1:].view(s.shape)
    off.copy_(s)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    a_in, b_in = s.clone().requires_grad_(True), off.detach().requires_grad_(True)
    a = S.sph_focal_loss([a_in], labels.cuda(), w_row.cuda(), avg_factor=4.0)
    b = S.sph_focal_loss([b_in], labels.cuda(), w_row.cuda(), avg_factor=4.0)
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(a))
    assert torch.equal(torch.autograd.grad(a, a_in)[0], torch.autograd.grad(b, b_in)[0])


@pytest.mark.parametrize('gamma,alpha', R.GAMMA_ALPHA)
def test_device_equals_host_twin(S, gamma, alpha):
    figures = {}
    x, labels = R.grid_inputs()
    dev = R.flat_loss_and_grads(S, x, labels, gamma, alpha, 'cuda')
    host = R.flat_loss_and_grads(S, x, labels, gamma, alpha, 'cpu')
    for name, d, h in zip(('loss', 'grad_two_pass', 'grad_fused'), dev, host):
        figures['grid ' + name] = (R.rel_err(d, h.double())[0], bool(torch.equal(d.cpu(), h)))
    scores, lab, w_row, _ = R.scene()
    outs = []
    for device in ('cuda', 'cpu'):
        ins = [s.clone().to(device).requires_grad_(True) for s in scores]
        loss = S.sph_focal_loss(ins, lab.to(device), w_row.to(device), gamma=gamma, alpha=alpha, avg_factor=5.0)
        outs.append(R.to_rows(torch.autograd.grad(loss, ins), 5).reshape(-1).cpu())
    figures['scene grad'] = (R.rel_err(outs[0], outs[1].double())[0], bool(torch.equal(outs[0], outs[1])))
    for name, (r, same) in figures.items():
        print(f'focal device vs host gamma={gamma} {name}: max rel {r:.3e} bit-equal {same}')
    for name, (r, same) in figures.items():
        assert r <= R.REL_GRID, (name, r)


def test_targets_loss_backward_capture_into_a_graph(S):
    """sph_anchor_targets -> sph_focal_loss(avg_factor=t.avg_factor) -> backward on the small scene: one stream, no parallel
    branches, nothing read back; two replays with changed logits equal the eager step bit for bit."""
    C = 5
    scores, _, _, _ = R.scene()
    B = scores[0].size(0)
    n = sum(s.size(1) // C * s.size(2) * s.size(3) for s in scores)
    g = torch.Generator().manual_seed(3)
    u = torch.rand((n, 4), generator=g)
    anchors = torch.stack([u[:, 0] * 360, 20 + u[:, 1] * 140, 5 + u[:, 2] * 60, 5 + u[:, 3] * 60], 1).cuda()
    counts = [4, 0, 3]
    k = sum(counts)
    pick = torch.randint(0, n, (k,), generator=g)
    gt = (anchors[pick.cuda()] + 0.5).contiguous()
    gt_labels = torch.randint(0, C, (k,), generator=g).cuda()
    offsets = torch.tensor([0, 4, 4, 7], dtype=torch.int64).cuda()
    assigner = S.SphMaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1,
                                   iou_calculator=dict(type='SphOverlaps2D', backend='sph2pob_standard_iou', box_version=4))
    ins = [s.cuda().requires_grad_(True) for s in scores]

    def step():
        t = S.sph_anchor_targets(anchors, gt, gt_labels, offsets, assigner=assigner, num_classes=C, k_max=4)
        loss = S.sph_focal_loss(ins, t.labels, t.label_weights, avg_factor=t.avg_factor)
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
