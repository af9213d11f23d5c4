"""The gate of tests/step_grad_cases.py, without a GPU: the restated step is the oracle's, the gate can fail, every case's
reference passes its own gate with figures near the default case's, and ``check`` obeys each of its rules."""
import pytest
import torch

from oracle import stage2 as o2
from tests import step_grad_cases as sg

OWN = [k for k, c in sg.CASES.items() if c['truth'] is None]  # the cases with a reference / truth of their own


def test_restated_step_gives_the_oracle_trainsteps_gradients():
    """Default case, fp32: step_gradients against o2.TrainStep.step in the state train_fix leaves behind iteration 5000.
    IDENTICAL, bit for bit (same modules, same order of operations; the dense table gradient of an index lookup holds the
    same sums as the sparse embedding's)."""
    ci, ref, _ = sg.case_data('default')
    conf = o2.bear_conf(**ci['conf_overrides'])
    net = o2.PSNetwork(conf)
    net.load_state_dict(ci['sd'])
    step = o2.TrainStep(net, conf, ci['light_init'].shape[0], ci['light_init'])
    step.train_fix()
    step.cur_iter = 5000
    step.train_fix()
    step.cur_iter = 5001
    step.step(ci['batch'][0], ci['batch'][1], ci['l_slt'], train_order=False, noise=ci['noise'])
    og = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    og['__light_dir'] = step.light_para.weight.grad.to_dense()
    og['__light_int'] = step.light_inten_para.weight.grad.to_dense()
    assert sorted(og) == sorted(ref)
    for k in og:
        assert torch.equal(og[k].double(), ref[k]), k


def test_restated_step_follows_train_fix_in_phase_one():
    """Phase 1 (train_fix at iteration 0): weights 0 / 0 / 0 / 10, BRDF nets and both tables frozen -- the oracle's own state."""
    ci, ref, truth = sg.case_data('phase1')
    conf = o2.bear_conf(**ci['conf_overrides'])
    net = o2.PSNetwork(conf)
    net.load_state_dict(ci['sd'])
    step = o2.TrainStep(net, conf, ci['light_init'].shape[0], ci['light_init'])
    step.step(ci['batch'][0], ci['batch'][1], ci['l_slt'], train_order=True, noise=ci['noise'])  # (the gradients precede the update)
    og = {k: p.grad for k, p in net.named_parameters() if p.requires_grad and p.grad is not None}
    assert sorted(og) == sorted(ref) == sorted(truth)
    assert not any(k.startswith(('albedo_net', 'rough_net', '__light')) for k in ref)
    for k in og:
        assert torch.equal(og[k].double(), ref[k]), k


@pytest.mark.parametrize('mutant', sg.MUTANTS)
def test_gate_rejects_mutant(mutant):
    """fp32 mutants of the restated step in place of the kernels' gradients: rejected, and at least one of the two figures lies
    10 x or more beyond the allowance.  Default case; 'masked_pixel' needs a surface pixel outside the object mask and runs on the
    default batch with every tenth surface pixel masked out ('mask_edge')."""
    case = 'mask_edge' if mutant == 'masked_pixel' else 'default'
    ci, ref, truth = sg.case_data(case)
    bad = sg.step_gradients(torch.float32, *sg.step_args(ci), light_init=ci['light_init'], mutant=mutant)
    m = sg.measure(bad, ref, truth)
    print(sg.report_line('mutant ' + mutant, m))
    assert m['bad']
    assert max(m['hip_t'] / (sg.FACTOR * m['E_t']), m['hip_r'] / (sg.FACTOR * m['E_r'])) >= 10.0
    with pytest.raises(AssertionError):
        sg.check(bad, ref, truth, 'mutant ' + mutant)


@pytest.mark.parametrize('name', OWN)
def test_reference_passes_its_own_gate(name):
    """Every case: the fp32 reference through the gate (trivially inside 8 x itself -- what is asserted is that names, zero
    tensors and finiteness hold), E_t and E_r finite and non-zero, and E_t within 10 x the default case's: beyond that, sign
    flips between fp32 and float64 have started to matter and the case needs another seed or size."""
    ci, ref, truth = sg.case_data(name)
    print('%s: %.0f %% of the pool\'s pixels are clear of every kink' % (name, 100 * ci['clear']))
    m = sg.check(ref, ref, truth, name)
    if name == 'no_surface':
        assert truth == {} and ref == {}
        return
    assert 0.0 < m['E_t'] < float('inf') and 0.0 < m['E_r'] < float('inf')
    e0 = sg.measure(*(sg.case_data('default')[k] for k in (1, 1, 2)))['E_t']
    assert m['E_t'] <= 10.0 * e0, '%s: E_t = %.2e, default case %.2e' % (name, m['E_t'], e0)
    n_surf = int(ci['batch'][0]['surface_mask'].sum())
    assert n_surf == sg.CASES[name]['Ns'] and ci['batch'][0]['surface_mask'].shape[1] == sg.CASES[name]['N'] and sg.CASES[name]['N'] % 4


def test_case_table_covers_the_launch_shapes():
    ns = sorted({c['Ns'] for c in sg.CASES.values()})
    assert all(k in ns for k in (0, 1, 63, 64, 65, 129, 541))
    assert {c['L'] for c in sg.CASES.values()} == {1, 3, 7} and {c['V'] for c in sg.CASES.values()} == {1, 2, 3}
    assert all(c['N'] <= 602 for c in sg.CASES.values())


# ---------------------------------------------------------------------------------------------------- unit checks of check
def _toy():
    g = torch.Generator().manual_seed(0)
    truth = {'w': torch.randn(6, 5, generator=g, dtype=torch.float64), 'b': torch.randn(5, generator=g, dtype=torch.float64)}
    truth['w'][2] *= 1e-5  # a tiny row: below the row floor, covered by the tensor form only
    truth['w'][4] *= 1e-2  # a small row above the floor: the row form is what sees a relative error there
    ref = {k: v * (1 + 1e-6 * torch.randn(v.shape, generator=g, dtype=torch.float64)) for k, v in truth.items()}
    hip = {k: v * (1 + 1e-6 * torch.randn(v.shape, generator=g, dtype=torch.float64)) for k, v in truth.items()}
    return hip, ref, truth


def test_check_passes_two_roundings_and_fails_a_large_error():
    hip, ref, truth = _toy()
    sg.check(hip, ref, truth, 'toy')
    hip['b'][3] += 1e-3 * truth['b'].abs().max()
    with pytest.raises(AssertionError, match='b: e_t'):
        sg.check(hip, ref, truth, 'toy')


def test_check_tiny_row_is_left_to_the_tensor_form():
    hip, ref, truth = _toy()
    s = float(truth['w'].abs().max())
    hip['w'][2, 0] += 2e-6 * s  # 20 % of that row's own size, 2e-6 of the tensor's: inside the tensor form, no row figure
    m = sg.check(hip, ref, truth, 'toy')
    assert m['hip_r'] < 1e-4
    hip['w'][2, 0] += 1e-3 * s  # ... but the tensor form does cover the row
    with pytest.raises(AssertionError, match='w: e_t'):
        sg.check(hip, ref, truth, 'toy')
    hip, ref, truth = _toy()
    hip['w'][4, 1] += 1e-4 * float(truth['w'][4].abs().max())  # 1e-6 of the tensor: only the row form objects
    assert sg.figures(hip['w'], truth['w'])[0] <= sg.FACTOR * sg.measure(ref, ref, truth)['E_t']
    with pytest.raises(AssertionError, match='w: e_r'):
        sg.check(hip, ref, truth, 'toy')


def test_check_all_zero_truth():
    hip, ref, truth = _toy()
    truth['z'] = torch.zeros(4, 3, dtype=torch.float64)
    ref['z'] = torch.zeros(4, 3)
    sg.check(hip, ref, truth, 'toy')                      # absent
    sg.check(dict(hip, z=None), ref, truth, 'toy')        # None
    sg.check(dict(hip, z=torch.zeros(4, 3)), ref, truth, 'toy')
    z = torch.zeros(4, 3)
    z[1, 1] = 1e-30
    with pytest.raises(AssertionError, match='z: truth is all zero, hip is not'):
        sg.check(dict(hip, z=z), ref, truth, 'toy')
    with pytest.raises(AssertionError, match='z: truth is all zero, ref is not'):
        sg.check(hip, dict(ref, z=z), truth, 'toy')


def test_check_nan_never_passes():
    hip, ref, truth = _toy()
    hip['w'][2, 2] = float('nan')  # in the tiny row: only the tensor form sees it
    with pytest.raises(AssertionError, match='w: e_t'):
        sg.check(hip, ref, truth, 'toy')
    hip, ref, truth = _toy()
    hip['b'][0] = float('nan')
    with pytest.raises(AssertionError, match='b: e_t'):
        sg.check(hip, ref, truth, 'toy')


def test_check_missing_and_extra_names():
    hip, ref, truth = _toy()
    with pytest.raises(AssertionError, match='b: no gradient'):
        sg.check({'w': hip['w']}, ref, truth, 'toy')
    with pytest.raises(AssertionError, match='b: no gradient'):
        sg.check(dict(hip, b=None), ref, truth, 'toy')
    sg.check(dict(hip, frozen=torch.zeros(3), other=None), ref, truth, 'toy')  # a frozen parameter: None or exactly zero
    with pytest.raises(AssertionError, match='frozen: a gradient the truth does not have'):
        sg.check(dict(hip, frozen=torch.full((3,), 1e-20)), ref, truth, 'toy')
