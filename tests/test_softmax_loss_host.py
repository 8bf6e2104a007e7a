"""CPU tier: the softmax cross-entropy, plain and mined, through the host twins (the row arithmetic, keys and cut rule the kernels
run, csrc/sph2pob_softmax.hpp) against the f64 truth of softmax_restatement.py, the scene semantics of `sph_softmax_loss`, and
the interface.  Measured maxima: DESIGN.md §4.11."""
import ctypes

import pytest
import torch

import softmax_restatement as R


@pytest.fixture(scope='module')
def S():
    import sph_retina_amd
    return sph_retina_amd


@pytest.mark.parametrize('k', (2, 6, 38))
def test_grid_accuracy_and_better_than_the_composition(S, k):
    R.check_grid(S, 'cpu', k)


def test_tails_are_finite_signed_and_close(S):
    R.check_tails(S, 'cpu')


def test_scene_mining_layouts_and_divisors(S):
    R.check_scene(S, 'cpu')


def test_scene_k38(S):
    R.check_k38(S, 'cpu')


def test_several_workgroups_scene(S):
    R.check_scene(S, 'cpu', levels=R.BIG_LEVELS, seed=R.BIG_SEED, need_cut=3)


def test_ties_take_the_lowest_rows(S):
    R.check_ties(S, 'cpu')


def test_plain_mode_function_and_module(S):
    R.check_plain_and_module(S, 'cpu')


@pytest.mark.parametrize('levels,seed', ((R.SCENE_LEVELS, R.SCENE_SEED), (R.BIG_LEVELS, R.BIG_SEED)))
def test_two_calls_give_the_same_bits(S, levels, seed):
    R.check_determinism(S, 'cpu', levels, seed)


def test_ties_over_several_chunks_of_the_walk(S):
    R.check_ties_over_several_chunks(S, 'cpu')


def test_ties_in_the_padded_tail_all_taken_and_all_but_one(S):
    R.check_ties_in_the_padded_tail(S, 'cpu')


def test_nan_loss_is_mined_first_and_reaches_the_sum(S):
    R.check_nan_loss_is_mined_first(S, 'cpu')


def test_class_levels_parses_nchw_flat_and_mixed_levels():
    """losses/_head.class_levels, which sph_focal_loss and sph_softmax_loss share: (H W per level, channels per anchor)."""
    from sph_retina_amd.losses import _head as H
    z = torch.zeros
    nchw = [z(2, 3 * 6, 4, 8), z(2, 2 * 6, 3, 5), z(2, 6, 1, 1)]            # n = 96 + 30 + 1
    flat = [z(2, 96, 6), z(2, 30, 6), z(2, 1, 6)]
    assert H.class_levels('f', 'K', nchw, 2, 127) == ([32, 15, 1], 6)
    assert H.class_levels('f', 'K', flat, 2, 127) == ([0, 0, 0], 6)
    assert H.class_levels('f', 'C', [nchw[0], flat[1], nchw[2]], 2, 127) == ([32, 0, 1], 6)
    assert H.class_levels('f', 'C', nchw, 2, 127, known_channels=6) == ([32, 15, 1], 6)
    # 18 channels x 32 positions: 6 channels for 96 anchors, or — told so by per-element weights — 9 for 64
    assert H.class_levels('f', 'C', nchw[:1], 2, 64, known_channels=9) == ([32], 9)
    with pytest.raises(ValueError, match=r'cls_scores\[1\]: expected \(B, A \* K, H, W\) or \(B, n_l, K\) with B = 2, got \(3, 12, 3, 5\)'):
        H.class_levels('f', 'K', [nchw[0], z(3, 12, 3, 5)], 2, 126)
    with pytest.raises(ValueError, match=r'cls_scores\[0\]: expected \(B, A \* C, H, W\) or \(B, n_l, C\) with B = 2, got \(2, 6\)'):
        H.class_levels('f', 'C', [z(2, 6)], 2, 1)
    with pytest.raises(ValueError, match=r'the class count differs across levels / weights: \[6, 7\]'):
        H.class_levels('f', 'K', [flat[0], z(2, 30, 7)], 2, 126)
    with pytest.raises(ValueError, match=r'the class count differs across levels / weights: \[5, 6\]'):
        H.class_levels('f', 'C', flat, 2, 127, known_channels=5)
    with pytest.raises(ValueError, match=r'the levels hold 756 scores per image, which 125 anchors \(labels.size\(1\)\) do not divide'):
        H.class_levels('f', 'K', nchw[:2], 2, 125)
    with pytest.raises(ValueError, match=r'the levels hold 756 scores per image, which 0 anchors'):
        H.class_levels('f', 'K', nchw[:2], 2, 0)
    with pytest.raises(ValueError, match='the class count must be positive'):
        H.class_levels('f', 'K', [z(2, 5, 0)], 2, 5)
    with pytest.raises(ValueError, match=r'cls_scores\[1\]: 12 channels are not a multiple of K = 7 \(K must be equal across levels\)'):
        H.class_levels('f', 'K', [z(2, 14, 4, 8), nchw[1], z(2, 4, 7)], 2, 130)
    with pytest.raises(ValueError, match=r'cls_scores\[0\]: 18 channels are not a multiple of C = 7 \(C must be equal across levels\)'):
        H.class_levels('f', 'C', nchw[:2], 2, 108)       # 756 = 108 x 7
    with pytest.raises(ValueError, match='the levels hold 126 anchors per image, labels 127'):
        H.class_levels('f', 'K', flat[:2], 2, 127)


def test_module_and_argument_errors(S):
    x, t = torch.randn(6, 5), torch.randint(0, 5, (6,))
    with pytest.raises(NotImplementedError, match='torch route'):
        S.CrossEntropyLoss(use_sigmoid=True)
    with pytest.raises(NotImplementedError, match='torch route'):
        S.CrossEntropyLoss(use_mask=True)
    m = S.CrossEntropyLoss(loss_weight=2.0)
    with pytest.raises(ValueError, match='avg_factor'):
        m(x, t, avg_factor=3.0, reduction_override='sum')
    with pytest.raises(AssertionError):
        m(x, t, reduction_override='max')
    want = 2.0 * float(torch.nn.functional.cross_entropy(x.double(), t))
    assert abs(float(m(x, t)) - want) <= 1e-5 * abs(want)
    assert m(x, t, reduction_override='none').shape == (6,)
    with pytest.raises(ValueError, match='weight'):
        m(x, t, torch.rand(7))
    with pytest.raises(ValueError, match='class_weight'):
        S.cross_entropy(x, t, class_weight=torch.ones(4))
    with pytest.raises(ValueError, match='integer labels'):
        S.cross_entropy(x, t.float())
    with pytest.raises(ValueError, match=r'\[2, 4096\]'):
        S.cross_entropy(torch.randn(6, 1), torch.zeros(6, dtype=torch.int64), reduction='sum')
    # N == 0
    x0, l0 = torch.zeros((0, 5), requires_grad=True), torch.zeros((0,), dtype=torch.int64)
    s0 = S.cross_entropy(x0, l0, reduction='sum')
    assert float(s0) == 0.0 and torch.autograd.grad(s0, x0)[0].shape == (0, 5)
    assert torch.isnan(S.cross_entropy(x0, l0, reduction='mean'))
    assert S.cross_entropy(x0, l0, reduction='none').shape == (0,)


def test_sph_softmax_loss_argument_errors(S):
    """The wording of sph_focal_loss's checks."""
    scores, labels, _ = R.scene()
    with pytest.raises(ValueError, match='cross_entropy'):
        S.sph_softmax_loss(scores, labels, reduction='none')
    with pytest.raises(ValueError, match='avg_factor'):
        S.sph_softmax_loss(scores, labels, reduction='sum', avg_factor=2.0)
    with pytest.raises(ValueError, match='anchors'):
        S.sph_softmax_loss(scores[:2], labels)                       # sum n_l != labels.size(1)
    with pytest.raises(ValueError, match='anchors'):
        S.sph_softmax_loss([R.to_rows([s]) for s in scores[:2]], labels)
    with pytest.raises(ValueError, match='class count'):
        S.sph_softmax_loss([R.to_rows([scores[0]]), torch.zeros(4, 31, 4)], labels)
    with pytest.raises(ValueError, match='levels'):
        S.sph_softmax_loss([scores[2]] * 9, labels[:, :9])
    with pytest.raises(RuntimeError, match='MI355X'):
        S.sph_softmax_loss([scores[0], scores[1].to('meta'), scores[2]], labels)
    with pytest.raises(ValueError, match='neg_pos_ratio'):
        S.sph_softmax_loss(scores, labels, neg_pos_ratio=-1)
    with pytest.raises(ValueError, match='neg_pos_ratio'):
        S.sph_softmax_loss(scores, labels, neg_pos_ratio=1.5)
    with pytest.raises(ValueError, match='label_weights'):
        S.sph_softmax_loss(scores, labels, torch.ones(4, 126))


def test_registry_builds_cross_entropy_loss_without_mmdet(S):
    from sph_retina_amd import registry
    if registry.LOSSES_IS_MMDET:
        assert registry.LOSSES.get('SphCrossEntropyLoss') is S.CrossEntropyLoss
        return
    m = registry.build_loss(dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    assert isinstance(m, S.CrossEntropyLoss) and m.use_sigmoid is False and m.loss_weight == 1.0


def test_abi_version_is_unchanged(S):
    from sph_retina_amd import _lib
    assert _lib.lib().sph2pob_abi_version() == 6


def test_c_entries_validate_before_touching_a_device(S):
    """Documented codes with NULL pointers and no GPU, device library and host twins alike."""
    from sph_retina_amd import _lib
    null = ctypes.c_void_p(0)
    one = (ctypes.c_int64 * 1)(4)
    bad = (ctypes.c_int64 * 1)(-1)
    hw3 = (ctypes.c_int64 * 1)(3)
    f = ctypes.c_float
    for lib, sfx in ((_lib.lib(), ''), (_lib.host_lib(), '_cpu')):
        total = getattr(lib, 'sph2pob_softmax_loss_sum_f32' + sfx)
        fwd = getattr(lib, 'sph2pob_softmax_loss_fwd_f32' + sfx)
        bwd = getattr(lib, 'sph2pob_softmax_loss_bwd_f32' + sfx)

        def tail(ratio=3):   # labels, weight, class_weight, ignore_index, background, ratio, scale, avg_factor, out, workspace, stream
            return (null, null, null, -100, 5, ratio, f(1.0), null, null, null, null)
        assert total(null, null, one, null, 1, 1, 6, *tail(-2)) == -3       # neg_pos_ratio < -1
        assert total(null, null, one, null, 0, 1, 6, *tail()) == -4         # no level
        assert total(null, null, one, null, 9, 1, 6, *tail()) == -4         # more than 8 levels
        assert total(null, null, one, null, 1, 1, 1, *tail()) == -4         # K = 1
        assert total(null, null, one, null, 1, 1, 4097, *tail()) == -4      # K = 4097
        assert total(null, null, one, null, 1, -1, 6, *tail()) == -4        # negative count
        assert total(null, null, null, null, 1, 1, 6, *tail()) == -1        # NULL tables
        assert total(null, null, one, null, 1, 1, 6, *tail()) == -1
        ptrs = (ctypes.c_void_p * 1)(0)
        assert total(ptrs, null, bad, null, 1, 1, 6, *tail()) == -4         # n_l < 0
        assert total(ptrs, null, one, hw3, 1, 1, 6, *tail()) == -4          # H W does not divide n_l
        assert total(ptrs, null, one, null, 1, 1, 6, *tail()) == -1         # a NULL logits entry with work to do
        assert total(ptrs, null, one, null, 1, 1, 6, *tail(-1)) == -1       # plain mode likewise
        assert fwd(null, null, null, null, -100, f(1.0), null, 0, 6, null) == 0          # n == 0: a no-op
        assert fwd(null, null, null, null, -100, f(1.0), null, 4, 6, null) == -1
        assert fwd(null, null, null, null, -100, f(1.0), null, -1, 6, null) == -4
        assert fwd(null, null, null, null, -100, f(1.0), null, 4, 1, null) == -4
        assert fwd(null, null, null, null, -100, f(1.0), null, 4, 4097, null) == -4
        assert bwd(null, null, null, null, -100, null, 0, f(1.0), null, null, 0, 6, null) == 0
        assert bwd(null, null, null, null, -100, null, 0, f(1.0), null, null, 4, 6, null) == -1
        assert bwd(null, null, null, null, -100, null, 2, f(1.0), null, null, 4, 6, null) == -3
        assert bwd(null, null, null, null, -100, null, 1, f(1.0), null, null, 4, 1, null) == -4
    lib = _lib.lib()
    plain, mining = (lib.sph2pob_softmax_loss_workspace_bytes(one, null, 1, 8, 38, m) for m in (0, 1))
    assert plain >= 16 and mining >= plain + 8 * 4 * 4
    assert lib.sph2pob_softmax_loss_workspace_bytes(bad, null, 1, 8, 38, 1) == 0
    assert lib.sph2pob_softmax_loss_workspace_bytes(one, null, 1, 8, 1, 1) == 0
    assert lib.sph2pob_softmax_loss_workspace_bytes(one, null, 1, 8, 4097, 0) == 0
    # empty levels write a zero sum (host twin: there is a device behind the other library only on the GPU tier)
    out, ws = (ctypes.c_float * 1)(7.0), (ctypes.c_double * 8)()
    zero = (ctypes.c_int64 * 1)(0)
    host = _lib.host_lib()
    assert host.sph2pob_softmax_loss_sum_f32_cpu(ptrs, null, zero, null, 1, 1, 6, null, null, null, -100, 5, 3, f(1.0), null, out, ws, null) == 0
    assert out[0] == 0.0
