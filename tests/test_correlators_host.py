"""The two-point observables on the host (CPU): the prefix-sum restatements of the two taxicab measurements, the
derived quantities and Links.* against the reference's own outputs (tests/golden/correlators.npz, made by
tools/make_golden_correlators.py from equilibrated reference chains).

The restatement: the reference gathers, per displacement and origin, the links of a fixed time-then-space
path (spin.py:128-222, vortex.py:147-187).  A periodic run of links is a difference of two prefix sums over the doubled
row or column, so with Pt / Px the prefix sums of the time / space component

    s = (Pt[bt + dt, x0] - Pt[bt, x0]) + xsign (Px[t0 + dt, bx + dx] - Px[t0 + dt, bx]),
    bt = t0 + off (+ N if dt < 0),  bx = x0 + off (+ N if dx < 0),

and the measurement is the mean over origins of exp(a s + b (|dt| + |dx|)).  The float error of s against the
reference's own sums is the rounding of two prefix sums of at most 2 N links: 4 * 2N * 2^-52 * M with M the largest
|prefix| -- which `taxicab_host` reports so that tests on larger lattices can bound the exponent's error by it.

Measured against the goldens (N = 5, 8, 16): at most 2.7e-14 relative (0.0 with the exact integer sums); the bound
asserted is the project's float standard, 1e-12.
"""
import numpy as np
import pytest

import supervillain_amd as sv
from supervillain_amd import observable as O
from supervillain_amd.lattice import Form, _fft_coordinates
from tests.golden import cases

CASES = cases('correlators.npz')
TAXICAB = [c for c in CASES if c['taxicab']]
RTOL = 1e-12


def action_of(c):
    L = sv.Lattice2D(c['N'])
    if c['kind'] == 'villain':
        return sv.Villain(L, c['kappa'], c['W'])
    return sv.Worldline(L, c['kappa'], float('inf') if c['W'] < 0 else c['W'])


def case_id(c):
    return f"{c['kind']}-N{c['N']}-W{c['W']}"


def taxicab_host(links, a, b, dual, W=None):
    """(out, M): the taxicab measurement of float links (2, N, N) from prefix sums, and the largest |prefix| entry.
    With W, `links` holds the integers W * Links: the prefix sums are exact and s is divided once."""
    links = np.asarray(links)
    N = links.shape[-1]
    tcomp, xcomp, off, xsign = (1, 0, 1, -1) if dual else (0, 1, 0, 1)
    zero = np.zeros((1, N), dtype=links.dtype)
    Pt = np.concatenate([zero, np.cumsum(np.concatenate([links[tcomp]] * 2, axis=0), axis=0)], axis=0)  # (2N+1, N)
    Px = np.concatenate([zero.T, np.cumsum(np.concatenate([links[xcomp]] * 2, axis=1), axis=1)], axis=1)  # (N, 2N+1)
    M = float(max(np.abs(Pt).max(), np.abs(Px).max()))
    coords = _fft_coordinates(N)
    t0 = np.arange(N)[:, None]
    x0 = np.arange(N)[None, :]
    out = np.zeros((N, N))
    for dt in coords:
        bt = t0 + off + (N if dt < 0 else 0)
        St = Pt[bt + dt, x0] - Pt[bt, x0]
        r = (t0 + dt) % N
        for dx in coords:
            bx = x0 + off + (N if dx < 0 else 0)
            Sx = Px[r, bx + dx] - Px[r, bx]
            s = St + xsign * Sx
            if W is not None:
                s = s / W
            out[dt, dx] = np.exp(a * s + b * (abs(dt) + abs(dx))).mean()
    out[0, 0] = 1
    return out, M


def taxicab_parameters(c):
    """(links, a, b, dual) of a golden case's taxicab measurement (spin.py:222, vortex.py:186-187)."""
    k = c['kappa']
    if c['kind'] == 'worldline':
        return c['Links'], -1 / k, -1 / (2 * k), 0
    return c['Links'], 2 * np.pi * k, -2 * np.pi * k * np.pi, 1


def taxicab_golden(c):
    return c['Spin_Spin'] if c['kind'] == 'worldline' else c['Vortex_Vortex']


def relative(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def test_fixture_covers_the_issue():
    kinds = {(c['kind'], c['N'], c['W']) for c in CASES}
    for N in (4, 5, 8, 16):
        assert {('villain', N, 1), ('villain', N, 2), ('worldline', N, 1), ('worldline', N, 2),
                ('worldline', N, -1)} <= kinds
    assert len(TAXICAB) == 15


@pytest.mark.parametrize('c', TAXICAB, ids=case_id)
def test_prefix_sum_restatement_equals_the_reference(c):
    links, a, b, dual = taxicab_parameters(c)
    got, M = taxicab_host(links, a, b, dual)
    want = taxicab_golden(c)
    assert np.isfinite(want).all() and M > 0
    err = relative(got, want)
    print(case_id(c), 'restatement vs reference: relative', err)
    assert err <= RTOL


@pytest.mark.parametrize('c', [c for c in TAXICAB if c['kind'] == 'worldline' and c['W'] > 0], ids=case_id)
def test_exact_integer_restatement(c):
    """Finite W: W Links = W m - delta(v) is an integer field; integer prefix sums, one division."""
    W = c['W']
    v, m = c['v'], c['m']
    WL = np.stack([W * m[0] - (v - np.roll(v, 1, axis=1)), W * m[1] + (v - np.roll(v, 1, axis=0))]).astype(np.int64)
    assert np.array_equal(WL / W, c['Links'])
    _, a, b, dual = taxicab_parameters(c)
    got, _ = taxicab_host(WL, a, b, dual, W=float(W))
    assert relative(got, taxicab_golden(c)) <= RTOL


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_links(c):
    S = action_of(c)
    L = S.Lattice
    if c['kind'] == 'villain':
        got = O.Links.Villain(S, Form(c['phi'][None], degree=0, lattice=L), Form(c['n'], degree=1, lattice=L))
    else:
        got = O.Links.Worldline(S, Form(c['m'], degree=1, lattice=L), Form(c['v'][None], degree=2, lattice=L))
    assert np.allclose(np.asarray(got), c['Links'], rtol=RTOL, atol=0)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_derived_quantities(c):
    S = action_of(c)
    for prefix in ('Spin', 'Vortex'):
        name = f'{prefix}_{prefix}'
        if name not in c:
            continue
        norm = getattr(O, f'{name}_Normalized').default(S, c[name])
        chi = getattr(O, f'{prefix}Susceptibility').default(S, norm)
        scaled = getattr(O, f'{prefix}SusceptibilityScaled').default(S, chi)
        moment = getattr(O, f'{prefix}CriticalMoment').default(S, norm)
        assert np.allclose(norm, c[f'{name}_Normalized'], rtol=RTOL, atol=0)
        for got, key in ((chi, f'{prefix}Susceptibility'), (scaled, f'{prefix}SusceptibilityScaled'),
                         (moment, f'{prefix}CriticalMoment')):
            assert abs(got - c[key]) <= RTOL * abs(c[key]), key


def test_critical_scaling_dimensions():
    L = sv.Lattice2D(4)
    assert O.Spin_Spin.CriticalScalingDimension(sv.Villain(L, 0.5, 2)) == 0.5
    assert O.Vortex_Vortex.CriticalScalingDimension(sv.Villain(L, 0.5, 2)) == 0.5
    Winf = sv.Worldline(L, 0.6, float('inf'))
    assert O.Spin_Spin.CriticalScalingDimension(Winf) == 1 / 0.6 / np.pi
    assert O.Vortex_Vortex.CriticalScalingDimension(Winf) == 4 * np.pi * 0.6


def test_dimension_conditions():
    S3 = sv.Villain(sv.Lattice(3, 4), 0.5, 1)
    links = np.zeros((3, 4, 4, 4))
    with pytest.raises(NotImplementedError):
        O.Vortex_Vortex.Villain(S3, links)
    with pytest.raises(NotImplementedError):
        O.Spin_Spin.Worldline(sv.Worldline(sv.Lattice(3, 4), 0.5, 1), links)
    with pytest.raises(NotImplementedError):
        O.Vortex_Vortex.Worldline(sv.Worldline(sv.Lattice(1, 4), 0.5, 1), np.zeros((1, 4)))


def test_ensemble_attributes_still_resolve_fields():
    S = sv.Villain(sv.Lattice2D(4), 0.5, 1)
    e = sv.Ensemble(S).from_configurations(S.configurations(3))
    assert e.phi.shape == (3, 1, 4, 4)
    with pytest.raises(AttributeError):
        e.no_such_field
    assert set(O.registry) == {'Links', 'Spin_Spin', 'Vortex_Vortex'}
    links = e.Links
    assert links.shape == (3, 2, 4, 4) and e.Links is links
