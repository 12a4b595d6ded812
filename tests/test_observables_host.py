"""The action, energy, winding and wrapping observables on the host (CPU) against the reference's own outputs
(tests/golden/observables.npz, made by tools/make_golden_observables.py), the packing identity behind the device's
one-pass pair of autocorrelations restated in NumPy, and the contact stencil of Winding_Winding.Worldline.

The packing identity (include/supervillain_amd.h): for real fields a, b and Z = fft2(a + i b),
    A(k) = (Z(k) + conj Z(-k)) / 2,   B(k) = (Z(k) - conj Z(-k)) / (2i),
    fft2(|A|^2 + i |B|^2) / V^2 = C_aa + i C_bb,   C_ff(r) = 1/V sum_x f(x) f(x - r).
Both sides are a few dozen float operations per element on unit-scale numbers; the bound is the project's float
standard, 1e-12, times the power of the fields, max(1, mean(a^2) + mean(b^2)).
"""
import numpy as np
import pytest

import supervillain_amd as sv
from supervillain_amd import observable as O
from supervillain_amd.lattice import Form
from tests.golden import cases

CASES = cases('observables.npz')
RTOL = 1e-12
SCALARS = ('ActionDensity', 'InternalEnergyDensity', 'InternalEnergyDensitySquared', 'WindingSquared')
NEW_PRIMARY = SCALARS + ('TorusWrapping', 'WrappingSquared', 'ActionTwoPoint', 'Winding_Winding')


def action_of(c):
    L = sv.Lattice2D(c['N'])
    if c['kind'] == 'villain':
        return sv.Villain(L, c['kappa'], c['W'])
    return sv.Worldline(L, c['kappa'], float('inf') if c['W'] < 0 else c['W'])


def case_id(c):
    return f"{c['kind']}-N{c['N']}-W{c['W']}-{c.get('source', 'random')}"


def scalar_arguments(c):
    """name -> the arguments after S of the formulation's static method, from a golden case's arrays."""
    if c['kind'] == 'villain':
        phi, n = c['phi'][None], c['n']
        return {'ActionDensity': (phi, n), 'InternalEnergyDensity': (phi, n), 'InternalEnergyDensitySquared': (phi, n),
                'WindingSquared': (n,), 'TorusWrapping': (phi, n)}
    links = c['Links']
    return {'ActionDensity': (links,), 'InternalEnergyDensity': (links,), 'InternalEnergyDensitySquared': (links,),
            'WindingSquared': (links,), 'TorusWrapping': (c['m'],)}


def host_scalars(c):
    S = action_of(c)
    method = 'Villain' if c['kind'] == 'villain' else 'Worldline'
    return {name: getattr(getattr(O, name), method)(S, *args) for name, args in scalar_arguments(c).items()}


def packed_fields(c):
    """(a, b, scale_bb): the two real fields whose autocorrelations a case's two-point functions are, formed on the
    host as the reference forms them, and the factor Winding_Winding applies to C_bb."""
    S = action_of(c)
    L, kappa = S.Lattice, S.kappa
    if c['kind'] == 'villain':
        a = 0.5 * kappa * (c['Links'] ** 2).sum(axis=0)
        b = np.asarray(O.d(Form(c['n'], degree=1, lattice=L)))[0].astype(float)
        return a, b, 1.0
    a = 1 - 0.5 / kappa * (c['Links'] ** 2).sum(axis=0)
    b = np.asarray(O.d(Form(c['Links'], degree=1, lattice=L)))[0]
    return a, b, 1 / (2 * np.pi * kappa) ** 2


def power_bound(a, b):
    """The bound of the two-point checks: 1e-12 for unit-power fields, scaled by the power of the packed fields."""
    return RTOL * max(1.0, float(np.mean(a ** 2) + np.mean(b ** 2)))


def definition(f):
    """C(r) = 1/V sum_x f(x) f(x - r), summed as written."""
    N = f.shape[0]
    out = np.empty((N, N))
    for dt in range(N):
        for dx in range(N):
            out[dt, dx] = np.mean(f * np.roll(f, (dt, dx), axis=(0, 1)))
    return out


def packed_correlations(a, b):
    """(C_aa, C_bb) from one transform of a + i b: the identity the device's power-spectrum load uses."""
    Z = np.fft.fft2(a + 1j * b)
    Zm = np.conj(np.roll(Z[::-1, ::-1], (1, 1), axis=(0, 1)))  # conj Z(-k)
    A, B = (Z + Zm) / 2, (Z - Zm) / 2j
    C = np.fft.fft2(np.abs(A) ** 2 + 1j * np.abs(B) ** 2) / a.size ** 2
    return C.real, C.imag


def two_point_from(c, C_aa, C_bb):
    """(ActionTwoPoint, Winding_Winding) of a golden case from the autocorrelations of its packed fields: the contact
    terms of action.py:99, :148-150 and winding.py:202."""
    S = action_of(c)
    kappa = S.kappa
    action = C_aa.copy()
    if c['kind'] == 'villain':
        action[0, 0] -= (0.5 * kappa * (c['Links'] ** 2).sum(axis=0)).mean()
        return action, C_bb
    action[0, 0] -= ((c['Links'] ** 2).sum(axis=0) / 2 / kappa).mean()
    return action, (kappa * O.Winding_Winding.contact(S.Lattice) - C_bb) / (2 * np.pi * kappa) ** 2


def test_fixture_covers_the_issue():
    kinds = {(c['kind'], c['N'], c['W']) for c in CASES}
    for N in (3, 4, 5, 8, 16):
        assert {('villain', N, 1), ('villain', N, 2), ('worldline', N, 2)} <= kinds
    for N in (4, 5, 8, 16):
        assert {('worldline', N, 1), ('worldline', N, 2), ('worldline', N, -1)} <= kinds
    for c in CASES:
        V = c['N'] ** 2
        if c['kind'] == 'villain' or c['source'] == 'random':
            assert (c['TorusWrapping'] != 0).all(), case_id(c)
        if c['kind'] == 'villain':
            dn = np.asarray(O.d(Form(c['n'], degree=1, lattice=sv.Lattice2D(c['N']))))
            assert np.count_nonzero(dn) >= V / 4
        elif c['N'] > 4:
            assert np.count_nonzero(np.asarray(O.d(Form(c['Links'], degree=1, lattice=sv.Lattice2D(c['N']))))) > 0


def test_the_new_observables_are_primary():
    for name in NEW_PRIMARY:
        assert name in O.primary and issubclass(O.primary[name], O.Observable), name
    for name in ('InternalEnergyDensityVariance', 'SpecificHeatCapacity', 'Action_Action'):
        assert issubclass(getattr(O, name), O.DerivedQuantity) and name not in O.primary


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_host_scalars_against_the_reference(c):
    S = action_of(c)
    got = host_scalars(c)
    for name in SCALARS:
        print(case_id(c), name, got[name], c[name])
        assert abs(got[name] - c[name]) <= RTOL * abs(c[name]), name
    assert np.array_equal(got['TorusWrapping'], c['TorusWrapping'])
    wrapping_squared = O.WrappingSquared.default(S, got['TorusWrapping'])
    assert abs(wrapping_squared - c['WrappingSquared']) <= RTOL * abs(c['WrappingSquared'])


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_derived_quantities_against_the_reference(c):
    S = action_of(c)
    variance = O.InternalEnergyDensityVariance.default(S, c['InternalEnergyDensitySquared'], c['InternalEnergyDensity'])
    assert abs(variance - c['InternalEnergyDensityVariance']) <= RTOL * abs(c['InternalEnergyDensityVariance'])
    heat = O.SpecificHeatCapacity.default(S, c['InternalEnergyDensityVariance'])
    assert abs(heat - c['SpecificHeatCapacity']) <= RTOL * abs(c['SpecificHeatCapacity'])
    aa = O.Action_Action.default(S, c['ActionTwoPoint'], c['ActionDensity'])
    assert np.abs(aa - c['Action_Action']).max() <= RTOL * max(1.0, np.abs(c['Action_Action']).max())


@pytest.mark.parametrize('N', [4, 5, 16])
def test_packing_identity_against_the_definition(N):
    r = np.random.default_rng(N)
    a, b = r.normal(size=(N, N)), r.integers(-3, 4, (N, N)).astype(float)
    C_aa, C_bb = packed_correlations(a, b)
    bound = power_bound(a, b)
    err = max(np.abs(C_aa - definition(a)).max(), np.abs(C_bb - definition(b)).max())
    print('N', N, 'packed pass vs definition: max |difference|', err, 'bound', bound)
    assert err <= bound


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_packed_restatement_against_the_reference(c):
    """The NumPy restatement of what the device computes reproduces the reference's two-point functions, whose own
    imaginary parts are round-off."""
    a, b, _ = packed_fields(c)
    bound = power_bound(a, b)
    action, winding = two_point_from(c, *packed_correlations(a, b))
    for got, name in ((action, 'ActionTwoPoint'), (winding, 'Winding_Winding')):
        want = c[name]
        err = np.abs(got - want.real).max()
        print(case_id(c), name, 'max |difference|', err, 'golden max |imag|', np.abs(want.imag).max(), 'bound', bound)
        assert err <= bound and np.abs(want.imag).max() <= bound, name


@pytest.mark.parametrize('N', [2, 3, 4, 5])
def test_contact_stencil_against_the_reference(N):
    """contact = ((2 pi kappa)^2 Winding_Winding.Worldline + C_bb) / kappa, C_bb by the definition; at small N the
    neighbours of the origin coincide and their entries add up."""
    L = sv.Lattice2D(N)
    contact = O.Winding_Winding.contact(L)
    want = np.zeros((N, N))
    for r, w in (((0, 0), 4), ((1, 0), -1), ((-1, 0), -1), ((0, 1), -1), ((0, -1), -1)):
        want[r[0] % N, r[1] % N] += w
    assert np.array_equal(contact, want)
    found = [c for c in CASES if c['kind'] == 'worldline' and c['N'] == N]
    assert found
    for c in found:
        kappa = c['kappa']
        _, b, _ = packed_fields(c)
        from_golden = ((2 * np.pi * kappa) ** 2 * c['Winding_Winding'].real + definition(b)) / kappa
        err = np.abs(from_golden - contact).max()
        print(case_id(c), 'contact from the golden: max |difference|', err)
        assert err <= 1e-12 * max(1.0, float(np.mean(b ** 2))) / kappa


def test_dimension_conditions():
    S1 = sv.Villain(sv.Lattice(1, 4), 0.5, 1)
    with pytest.raises(NotImplementedError):
        O.WindingSquared.Villain(S1, np.zeros((1, 4), dtype=int))
    with pytest.raises(NotImplementedError):
        O.Winding_Winding.Villain(S1, np.zeros((1, 4), dtype=int))
    S3 = sv.Worldline(sv.Lattice(3, 4), 0.5, 1)
    with pytest.raises(NotImplementedError):
        O.ActionTwoPoint.Worldline(S3, np.zeros((3, 4, 4, 4)))


def test_measure_resolves_default_and_inline_columns():
    """observable.measure resolves an observable that only has `default` from its arguments, and returns a column the
    configurations already hold as it is."""
    S = sv.Villain(sv.Lattice2D(4), 0.5, 1)
    cfgs = S.configurations(3)
    n = np.random.default_rng(5).integers(-2, 3, (3, 2, 4, 4))
    for i in range(3):
        cfgs[i] = {'phi': np.zeros((1, 4, 4)), 'n': n[i]}
    e = sv.Ensemble(S).from_configurations(cfgs)
    tw = e.TorusWrapping
    assert tw.shape == (3, 2) and np.array_equal(np.asarray(tw), n.sum(axis=(2, 3)))
    ws = e.WrappingSquared
    assert ws.shape == (3,) and np.array_equal(np.asarray(ws), (n.sum(axis=(2, 3)) ** 2).sum(axis=1))
    assert e.WrappingSquared is ws and e.TorusWrapping is tw
    w2 = e.WindingSquared
    assert w2.shape == (3,)
    for i in range(3):
        assert w2[i] == O.WindingSquared.Villain(S, n[i])
