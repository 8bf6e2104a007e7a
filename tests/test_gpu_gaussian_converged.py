"""GPU: the Gaussian losses in the converged regime on the device, with the CPU tier's check functions, bounds and cached
references (tests/test_gaussian_converged_host.py holds the checks and the measured table, tests/gaussian_converged_scenes.py
the scenes, masks, float64 truth and float32 yardstick), and the device against its host twin."""
import numpy as np
import pytest

import gaussian_converged_scenes as S
import test_gaussian_converged_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['fast', 'reference'])
def arith(request):
    import sph_retina_amd as A
    A.set_arithmetic(request.param)
    yield request.param
    A.set_arithmetic('fast')


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.TIERS)
def test_values_gradients_exact_rows_vs_fp64(tier, box, arith):
    worst = H.converged_checks('cuda', tier, box, arith)
    print(f'MI355X {tier} {box} {arith}: ' + ' '.join(f'{x:.2f}' for x in worst))


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.SYM_TIERS)
def test_symmetric_kld_selection(tier, box, arith):
    H.selection_checks('cuda', tier, box, arith)


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('name', ['kld-sqrt-log1p1', 'kf-ln'])
def test_sizes_tails_sentinels_weights_and_sums(box, name):
    H.size_checks('cuda', box, name)


@pytest.mark.parametrize('box', S.BOXES)
@pytest.mark.parametrize('tier', S.TIERS)
def test_device_against_host_twin(tier, box, arith):
    """One source for both: the same NaN pattern (none), the same exactly-zero gradient rows, and on the decisive rows of
    kld_symmax / kld_symmin the same selection (`selection_checks` holds each side to the branch float64 selects; here the two
    gradient rows are also nearer to each other than either is to the other branch)."""
    for cfg in S.cells(tier):
        pred, target = S.scene(tier, box, S.family_of(cfg))
        dev, twin = (H.call(d, pred, target, cfg['tail'], arith) for d in ('cuda', 'cpu'))
        what = (tier, box, arith, cfg['name'])
        for k in ('loss', 'gp', 'gt'):
            assert np.array_equal(np.isnan(dev[k]), np.isnan(twin[k])), what + (k, 'NaN pattern')
        zd = (dev['gp'] == 0).all(1) & (dev['gt'] == 0).all(1)
        zt = (twin['gp'] == 0).all(1) & (twin['gt'] == 0).all(1)
        assert np.array_equal(zd, zt), what + ('zero rows', np.flatnonzero(zd != zt)[:5].tolist())
        if S.family_of(cfg) == 'sym':
            ref = S.reference(tier, box, cfg['name'])
            rows = ref['grad_mask'] & ~ref['zero_rows']
            as_ref = dict(gp=twin['gp'].astype(np.float64), gt=twin['gt'].astype(np.float64))
            other = dict(gp=ref['gp_other'], gt=ref['gt_other'])
            apart = S.row_error(ref['gp_other'], ref['gt_other'], ref) > 0.1
            rows &= apart
            assert (S.row_error(dev['gp'], dev['gt'], as_ref)[rows] < S.row_error(dev['gp'], dev['gt'], other)[rows]).all(), what
