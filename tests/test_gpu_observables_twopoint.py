"""Device ActionTwoPoint and Winding_Winding of both formulations (one transform pass of the packed fields,
supervillain_amd/csrc/correlators.hip) and the resident scalar observables, against the reference's outputs
(tests/golden/observables.npz), against host NumPy and against each other.

Bound of every two-point check: |got - want| <= 1e-12 * max(1, mean(a^2) + mean(b^2)) per element, the project's
1e-12 for unit-power fields scaled by the power of the packed fields a + i b (tests/test_observables_host.py).  A
sum over all V displacements carries V times that.  Float scalars: 1e-12 relative; integer ones: equality.
"""
import ctypes

import numpy as np
import pytest

import supervillain_amd as sv
from supervillain_amd import _native
from supervillain_amd import observable as O
from supervillain_amd._abi import SvWorldlineSums
from supervillain_amd.generator.combining import Sequentially
from supervillain_amd.lattice import Form
from tests.test_gpu_correlators import chain_of, fields_of, generator_for, is_pow2
from tests.test_observables_host import (CASES, NEW_PRIMARY, RTOL, SCALARS, action_of, case_id, host_scalars,
                                         packed_fields, power_bound, scalar_arguments)

pytestmark = pytest.mark.gpu

def displacements(N):
    """The eight displacements of test_fft_path_at_4096 (there N = 4096), its halves of N taken of this N."""
    h = N // 2
    return ((0, 1), (1, 0), (h, h), (-1, 3), (5, -7), (0, h), (1000, 17), (-h, h - 1))


def links_of(S, cfg):
    L = S.Lattice
    if isinstance(S, sv.Villain):
        return np.asarray(O.Links.Villain(S, Form(cfg['phi'], degree=0, lattice=L), Form(cfg['n'], degree=1, lattice=L)))
    return np.asarray(O.Links.Worldline(S, Form(cfg['m'], degree=1, lattice=L), Form(cfg['v'], degree=2, lattice=L)))


def packed_fields_of(S, cfg):
    """packed_fields for a downloaded configuration."""
    kind = 'villain' if isinstance(S, sv.Villain) else 'worldline'
    return packed_fields(dict(kind=kind, N=S.Lattice.N, kappa=S.kappa, W=S.W if S.W < float('inf') else -1,
                              Links=links_of(S, cfg), n=cfg.get('n')))


def one_shot(S, c, path):
    if c['kind'] == 'villain':
        return O.ActionTwoPoint.Villain(S, c['Links'], path=path), O.Winding_Winding.Villain(S, c['n'], path=path)
    return O.ActionTwoPoint.Worldline(S, c['Links'], path=path), O.Winding_Winding.Worldline(S, c['Links'], path=path)


def definition_at(f, r):
    return float(np.mean(f * np.roll(f, r, axis=(0, 1))))  # 1/V sum_x f(x) f(x - r)


def host_correlation(f):
    F = np.fft.fft2(f)
    return np.fft.ifft2(np.abs(F) ** 2).real / f.size


# ---- against the reference -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_two_point_functions_against_the_reference(c):
    S = action_of(c)
    N = c['N']
    a, b, _ = packed_fields(c)
    bound = power_bound(a, b)
    want = {'ActionTwoPoint': c['ActionTwoPoint'], 'Winding_Winding': c['Winding_Winding']}
    for name, w in want.items():
        assert np.abs(w.imag).max() <= bound, f'the imaginary part of the golden {name}'
    chain = chain_of(S, fields_of(c))
    worst = 0.0
    for path in (1, 2) if is_pow2(N) and N >= 4 else (1,):
        shot = one_shot(S, c, path)
        pair = O.action_winding(chain, path=path)
        alone = (O.ActionTwoPoint.resident(chain, path=path), O.Winding_Winding.resident(chain, path=path))
        for got, how in ((shot, 'one-shot'), (pair[:2], 'resident pair'), (alone, 'resident alone')):
            for g, name in zip(got, want):
                assert g.shape == (N, N) and g.dtype == np.float64
                err = np.abs(g - want[name].real).max()
                worst = max(worst, err)
                assert err <= bound, f'{case_id(c)} path {path} {how} {name}: {err} > {bound}'
        # identities, configuration by configuration
        winding_squared = host_scalars(c)['WindingSquared']
        assert abs(pair[1][0, 0] - winding_squared) <= bound
        if c['kind'] == 'villain':
            assert abs(pair[1].sum()) <= N * N * bound  # (sum dn)^2 / V = 0 on a torus
            assert abs(pair[0][0, 0] + a.mean() - np.mean(a ** 2)) <= bound
    print(case_id(c), 'largest |device - reference|', worst, 'bound', bound)
    chain.close()


# ---- the packed pass against single-field passes and np.fft ---------------------------------------------------------

@pytest.mark.parametrize('N', [64, 256])
def test_packed_pass_against_single_field_passes_and_numpy(N):
    L = sv.Lattice2D(N)
    S = sv.Villain(L, 0.5, 1)
    r = np.random.default_rng(N)
    cfg = {'phi': r.uniform(-np.pi, np.pi, (1, N, N)), 'n': r.integers(-2, 3, (2, N, N)).astype(np.int64)}
    a, b, _ = packed_fields_of(S, cfg)
    bound = power_bound(a, b)
    chain = chain_of(S, cfg)
    action, winding, _ = O.action_winding(chain, path=2)
    chain.close()
    action[0, 0] += a.mean()  # (the contact term off: the plain autocorrelation)
    packed = O.correlation_real(L, a, b, path=2)
    single = (O.correlation_real(L, a, path=2), O.correlation_real(L, b, path=2))
    numpy = (host_correlation(a), host_correlation(b))
    others = [('one-shot packed', packed), ('single-field passes', single), ('np.fft', numpy)]
    if N == 64:
        others.append(('direct sum', O.correlation_real(L, a, b, path=1)))
        assert np.array_equal(O.correlation_real(L, a, b, path=0)[0], packed[0])  # auto takes the FFT where it can
    for how, (w_aa, w_bb) in others:
        err = max(np.abs(action - w_aa).max(), np.abs(winding - w_bb).max())
        print(f'N={N} resident packed pass vs {how}: max |difference|', err, 'bound', bound)
        assert err <= bound, how


# ---- the largest rows ------------------------------------------------------------------------------------------------

def check_against_the_definition(S, chain, cfg):
    N = S.Lattice.N
    a, b, scale = packed_fields_of(S, cfg)
    bound = power_bound(a, b)
    action, winding, _ = O.action_winding(chain, path=2)
    worldline = isinstance(S, sv.Worldline)
    contact = O.Winding_Winding.contact(S.Lattice)
    for C, f, name in ((action, a, 'ActionTwoPoint'), (winding, b, 'Winding_Winding')):
        mirrored = np.roll(C[::-1, ::-1], (1, 1), axis=(0, 1))  # C(-r)
        err = np.abs(mirrored - C).max()
        print(name, 'max |C(-r) - C(r)|', err, 'bound', bound)
        assert err <= bound
        for r in displacements(N):
            assert r[0] % N or r[1] % N  # (no displacement is the origin, where ActionTwoPoint has its contact term)
            want, got = definition_at(f, r), C[r[0] % N, r[1] % N]
            if worldline and name == 'Winding_Winding':
                want = (S.kappa * contact[r[0] % N, r[1] % N] - want) * scale  # (winding.py:202)
            print(name, r, got, want)
            assert abs(got - want) <= bound, (name, r)


def test_fft_path_at_4096_villain():
    """The mirrored power-spectrum load on one 64 KiB row per workgroup, on an uploaded random (phi, n)."""
    N = 4096
    S = sv.Villain(sv.Lattice2D(N), 0.5, 1)
    r = np.random.default_rng(N)
    cfg = {'phi': r.uniform(-np.pi, np.pi, (1, N, N)), 'n': r.integers(-2, 3, (2, N, N)).astype(np.int64)}
    chain = chain_of(S, cfg)
    try:
        check_against_the_definition(S, chain, cfg)
    finally:
        chain.close()


def test_fft_path_at_1024_worldline_exact():
    """The integer field formation (W l, d(W l) as int64) after a few device steps."""
    N = 1024
    S = sv.Worldline(sv.Lattice2D(N), 0.5, 2)
    chain = chain_of(S, sweeps=3, seed=N)
    try:
        chain.advance()
        cfg = {k: np.array(x) for k, x in chain.download().items()}
        assert O.sums(chain)['exact'] == 1
        check_against_the_definition(S, chain, cfg)
    finally:
        chain.close()


# ---- resident scalars ------------------------------------------------------------------------------------------------

def assert_scalars(got, want, what):
    assert set(got) == set(SCALARS) | {'TorusWrapping'}
    for name in SCALARS:
        print(what, name, got[name], want[name])
        assert abs(got[name] - want[name]) <= RTOL * abs(want[name]), (what, name)
    assert np.array_equal(got['TorusWrapping'], want['TorusWrapping']), what


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_resident_scalars_against_the_host_forms(c):
    S = action_of(c)
    chain = chain_of(S, fields_of(c))
    want = host_scalars(c)
    assert_scalars(O.scalars(chain), want, case_id(c))
    assert_scalars(O.action_winding(chain)[2], want, case_id(c) + ' with the two-point functions')
    for name in SCALARS:
        assert abs(want[name] - c[name]) <= RTOL * abs(c[name])  # (and so against the reference)
    raw = O.sums(chain)
    if c['kind'] == 'villain':
        dn = np.asarray(O.d(Form(c['n'], degree=1, lattice=S.Lattice)))
        assert raw['dn2'] == int((dn ** 2).sum()) and [raw['n0'], raw['n1']] == list(c['n'].sum(axis=(1, 2)))
    else:
        assert [raw['m0'], raw['m1']] == list(c['m'].sum(axis=(1, 2)))
        assert raw['exact'] == (1 if c['W'] > 0 else 0)
        if c['W'] > 0:  # W l = W m - delta(v) and d(W l) are integers: their sums of squares are exact
            W, m, v = c['W'], c['m'], c['v']
            WL = np.stack([W * m[0] - (v - np.roll(v, 1, axis=1)), W * m[1] + (v - np.roll(v, 1, axis=0))])
            dWL = np.asarray(O.d(Form(WL, degree=1, lattice=S.Lattice)))
            assert raw['w_links_squared'] == int((WL ** 2).sum()) and raw['w_curl_squared'] == int((dWL ** 2).sum())
    chain.close()


@pytest.mark.parametrize('c', [c for c in CASES if c['kind'] == 'worldline' and c['W'] > 0 and c['N'] in (5, 16)],
                         ids=case_id)
def test_worldline_integer_path_equals_the_float_path(c):
    """The same (m, v) held as float v takes the float field formation and the ordered float sums."""
    S = action_of(c)
    N, lib = c['N'], _native.lib()
    chain = chain_of(S, fields_of(c))
    exact = O.action_winding(chain, path=1)
    exact_sums = O.sums(chain)
    h = ctypes.c_void_p()
    ctx = chain.ctx
    ctx.check(lib.sv_worldline_create(ctx.handle, N, 1, ctypes.byref(h)), 'sv_worldline_create')
    try:
        m, v = np.ascontiguousarray(c['m']), np.ascontiguousarray(c['v'].astype(np.float64))
        ctx.check(lib.sv_worldline_upload(h, _native.ptr(m), _native.ptr(v)), 'sv_worldline_upload')
        action, winding = np.empty((N, N)), np.empty((N, N))
        sums = SvWorldlineSums()
        ctx.check(lib.sv_worldline_action_winding(h, float(S.kappa), float(S._W), _native.ptr(action), _native.ptr(winding),
                                                  ctypes.byref(sums), 1), 'sv_worldline_action_winding')
    finally:
        ctx.check(lib.sv_worldline_destroy(h), 'sv_worldline_destroy')
    chain.close()
    assert exact_sums['exact'] == 1 and sums.exact == 0
    assert (sums.m0, sums.m1) == (exact_sums['m0'], exact_sums['m1'])
    for name in ('links_squared', 'curl_squared'):
        assert abs(getattr(sums, name) - exact_sums[name]) <= RTOL * abs(exact_sums[name]), name
    a, b, _ = packed_fields(c)
    bound = power_bound(a, b)
    assert np.abs(action - exact[0]).max() <= bound and np.abs(winding - exact[1]).max() <= bound


# ---- the measurements leave the chain alone ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['villain', 'worldline'])
def test_measuring_does_not_disturb_the_chain(kind):
    L = sv.Lattice2D(16)
    S = sv.Villain(L, 0.5, 2) if kind == 'villain' else sv.Worldline(L, 0.5, 2)

    def run(measure):
        chain = chain_of(S, sweeps=5, seed=77)
        chain.advance()
        if measure:
            for path in (0, 1, 2):
                O.action_winding(chain, path=path)
                O.ActionTwoPoint.resident(chain, path=path)
                O.Winding_Winding.resident(chain, path=path)
            O.scalars(chain)
            O.sums(chain)
        chain.advance()
        cfg = {k: np.array(x) for k, x in chain.download().items()}
        G = chain.generator
        leaves = G.generators if isinstance(G, Sequentially) else [G]
        counters = [(g.accepted, g.proposed, g.acceptance) for g in leaves]
        state = leaves[0].rng.bit_generator.state
        chain.close()
        return cfg, counters, state

    plain, measured = run(False), run(True)
    for k in plain[0]:
        assert np.array_equal(plain[0][k], measured[0][k]), k
    assert plain[1] == measured[1]
    assert plain[2] == measured[2]


# ---- Ensemble attributes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['villain', 'worldline'])
def test_ensemble_attributes(kind):
    steps, N = 4, 8
    L = sv.Lattice2D(N)
    S = sv.Villain(L, 0.5, 2) if kind == 'villain' else sv.Worldline(L, 0.5, 2)
    e = sv.Ensemble(S).generate(steps, generator_for(S, seed=8))
    shapes = {name: (steps,) for name in SCALARS + ('WrappingSquared',)}
    shapes |= {'TorusWrapping': (steps, 2), 'ActionTwoPoint': (steps, N, N), 'Winding_Winding': (steps, N, N)}
    assert set(shapes) == set(NEW_PRIMARY)
    got = {name: getattr(e, name) for name in NEW_PRIMARY}
    for name, x in got.items():
        assert x.shape == shapes[name], name
        assert getattr(e, name) is x, name
    for i in range(steps):
        cfg = e.configuration[i]
        links = O.Links.Villain(S, cfg['phi'], cfg['n']) if kind == 'villain' else O.Links.Worldline(S, cfg['m'], cfg['v'])
        c = dict(kind=kind, N=N, kappa=S.kappa, W=S.W, Links=np.asarray(links)) | {k: np.asarray(x) for k, x in cfg.items()}
        c |= {'phi': np.asarray(cfg['phi'])[0]} if kind == 'villain' else {}
        for name, args in scalar_arguments(c).items():
            want = getattr(getattr(O, name), 'Villain' if kind == 'villain' else 'Worldline')(S, *args)
            assert np.array_equal(got[name][i], want), name
        assert got['WrappingSquared'][i] == O.WrappingSquared.default(S, got['TorusWrapping'][i])
        for g, w in zip((got['ActionTwoPoint'][i], got['Winding_Winding'][i]), one_shot(S, c, 0)):
            assert np.array_equal(g, w)


def test_a_villain_inline_column_is_returned_as_it_is():
    S = sv.Villain(sv.Lattice2D(8), 0.5, 1)
    G = sv.generator.villain.NeighborhoodUpdate(S, device=0, inline=True)
    G.rng = np.random.default_rng(9)
    e = sv.Ensemble(S).generate(3, G)
    fields = e.configuration.fields
    for name in ('ActionDensity', 'InternalEnergyDensity', 'WindingSquared', 'TorusWrapping'):
        assert name in fields and name not in e.__dict__
        assert np.array_equal(np.asarray(getattr(e, name)), np.asarray(fields[name])), name
        assert name not in e.__dict__
    assert e.WrappingSquared.shape == (3,)
    assert np.array_equal(np.asarray(e.WrappingSquared), (np.asarray(fields['TorusWrapping']) ** 2).sum(axis=1))


# ---- sizes no path serves ------------------------------------------------------------------------------------------

def test_unsupported_sizes_raise_not_implemented():
    with pytest.raises(NotImplementedError, match='FFT'):
        O.correlation_real(sv.Lattice2D(96), np.ones((96, 96)), path=2)
    S = sv.Villain(sv.Lattice2D(96), 0.5, 1)
    with pytest.raises(NotImplementedError, match='FFT'):
        O.Winding_Winding.Villain(S, np.zeros((2, 96, 96), dtype=int), path=2)
    for path in (0, 1, 2):
        with pytest.raises(NotImplementedError, match='320'):
            O.correlation_real(sv.Lattice2D(320), np.ones((320, 320)), np.ones((320, 320)), path=path)
    Sw = sv.Worldline(sv.Lattice2D(320), 0.5, 1)
    chain = chain_of(Sw)
    for path in (0, 1, 2):
        with pytest.raises(NotImplementedError, match='320'):
            O.action_winding(chain, path=path)
    chain.close()
