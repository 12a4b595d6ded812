"""Device Spin_Spin and Vortex_Vortex of both formulations (supervillain_amd/csrc/correlators.hip) against the
reference's outputs (tests/golden/correlators.npz), against host NumPy and against each other.

Bounds.  Direct pair: |device - reference| <= 1e-12 |C(0)| per element, |C(0)| = 1, real and imaginary parts.
Taxicab pair: 1e-12 relative per element against the goldens; on the larger device-generated lattices the exact
integer path keeps 1e-12 and the float cases use the bound of tests/test_correlators_host.py, the rounding of two
prefix sums of at most 2 N links carried into the exponent: 4 |a| 2N 2^-52 M + 16 * 2^-52, M the largest |prefix|.
"""
import numpy as np
import pytest

import supervillain_amd as sv
from supervillain_amd import _native
from supervillain_amd import observable as O
from supervillain_amd.generator.combining import KeepEvery, Sequentially
from supervillain_amd.lattice import Form
from supervillain_amd.pipeline import DeviceChain, device_program
from tests.golden import cases
from tests.test_correlators_host import (TAXICAB, action_of, case_id, taxicab_golden, taxicab_host,
                                         taxicab_parameters)

pytestmark = pytest.mark.gpu

CASES = cases('correlators.npz')
TOL = 1e-12
EPS = 2.0 ** -52


def is_pow2(N):
    return N & (N - 1) == 0


def direct_golden(c):
    return c['Spin_Spin'] if c['kind'] == 'villain' else c['Vortex_Vortex']


def generator_for(S, seed=1):
    """A device generator of the action's formulation (a Worldline Hammer's two local updates share one rng)."""
    if isinstance(S, sv.Villain):
        G = sv.generator.villain.NeighborhoodUpdate(S, device=0)
        G.rng = np.random.default_rng(seed)
        return G
    P = sv.generator.worldline.PlaquetteUpdate(S, mode='checkerboard', device=0)
    C = sv.generator.worldline.CoexactUpdate(S, device=0)
    P.rng = C.rng = np.random.default_rng(seed)
    return Sequentially([P, C])


def chain_of(S, cfg=None, sweeps=1, seed=1):
    """A DeviceChain of S holding cfg (or a cold start); one advance() runs `sweeps` steps of generator_for(S)."""
    G = generator_for(S, seed)
    chain = DeviceChain(S, device_program(KeepEvery(sweeps, G) if sweeps > 1 else G))
    chain.upload(cfg if cfg is not None else S.configurations(1)[0])
    chain.generator = G
    return chain


def fields_of(c):
    if c['kind'] == 'villain':
        return {'phi': c['phi'][None], 'n': c['n']}
    return {'m': c['m'], 'v': c['v'][None]}


def assert_close_complex(got, want, what):
    err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    print(what, 'max |difference|', err)
    assert err <= TOL, what


def assert_relative(got, want, rtol, what):
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    nz = want != 0
    err = float(np.max(np.abs(got - want)[nz] / np.abs(want)[nz])) if nz.any() else 0.0
    print(what, 'max relative difference', err, 'bound', rtol)
    assert (np.abs(got - want) <= rtol * np.abs(want)).all(), what


def host_correlation(f):
    """Lattice.correlation(f, f) with np.fft (compact.py:465-...): fft(conj fft(f) fft(f)) / sqrt(V), ortho."""
    F = np.fft.fft2(f, norm='ortho')
    return np.fft.fft2(np.conj(F) * F, norm='ortho') / np.sqrt(f.size)


# ---- the direct pair -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_direct_pair_against_the_reference(c):
    S = action_of(c)
    N, want = c['N'], direct_golden(c)
    chain = chain_of(S, fields_of(c))
    for path in (1, 2) if is_pow2(N) else (1,):
        if c['kind'] == 'villain':
            one_shot = O.Spin_Spin.Villain(S, c['phi'][None], path=path)
            resident = O.Spin_Spin.resident(chain, path=path)
        else:
            one_shot = O.Vortex_Vortex.Worldline(S, c['v'][None], path=path)
            resident = O.Vortex_Vortex.resident(chain, path=path)
        for got, how in ((one_shot, 'one-shot'), (resident, 'resident')):
            assert got.shape == (N, N) and got.dtype == np.complex128
            assert_close_complex(got, want, f'{case_id(c)} path {path} {how}')
            assert abs(got[0, 0] - 1) <= TOL
    chain.close()


@pytest.mark.parametrize('N', [64, 256])
def test_fft_path_against_direct_sum_and_numpy(N):
    L = sv.Lattice2D(N)
    f = np.exp(1j * np.random.default_rng(N).uniform(-np.pi, np.pi, (N, N)))
    fft = O.correlation(L, f, path=2)
    direct = O.correlation(L, f, path=1)
    assert np.array_equal(O.correlation(L, f, path=0), fft)  # auto takes the FFT where it can
    assert_close_complex(fft, direct, f'N={N} FFT vs direct sum')
    assert_close_complex(fft, host_correlation(f), f'N={N} FFT vs np.fft')
    assert_close_complex(direct, host_correlation(f), f'N={N} direct sum vs np.fft')


def test_fft_path_at_4096():
    """The largest LDS footprint (one 64 KiB row per workgroup), on a configuration from a few device sweeps."""
    N = 4096
    S = sv.Villain(sv.Lattice2D(N), 0.5, 1)
    chain = chain_of(S, sweeps=3, seed=4096)
    chain.advance()
    C = O.Spin_Spin.resident(chain, path=2)
    f = np.exp(1j * chain.download()['phi'][0])
    chain.close()
    assert abs(C[0, 0] - 1) <= TOL
    mirrored = np.roll(C[::-1, ::-1], (1, 1), axis=(0, 1))  # C(-r)
    assert_close_complex(mirrored, np.conj(C), 'C(-r) = conj C(r)')
    for r in ((0, 1), (1, 0), (N // 2, N // 2), (-1, 3), (5, -7), (0, N // 2), (1000, 17), (-2048, 2047)):
        want = np.mean(np.conj(f) * np.roll(f, r, axis=(0, 1)))  # 1/V sum_x conj f(x) f(x - r)
        got = C[r[0] % N, r[1] % N]
        print(r, got, want)
        assert abs(got.real - want.real) <= TOL and abs(got.imag - want.imag) <= TOL, r


# ---- the taxicab pair ------------------------------------------------------------------------------------------

def taxicab_one_shot(S, links):
    return O.Spin_Spin.Worldline(S, links) if isinstance(S, sv.Worldline) else O.Vortex_Vortex.Villain(S, links)


def taxicab_resident(chain):
    return O.Spin_Spin.resident(chain) if chain.kind == 'worldline' else O.Vortex_Vortex.resident(chain)


def set_units(chain, units):
    chain.ctx.check(_native.lib().sv_ctx_set_taxicab_units(chain.ctx.handle, units), 'sv_ctx_set_taxicab_units')


@pytest.mark.parametrize('c', TAXICAB, ids=case_id)
def test_taxicab_pair_against_the_reference(c):
    S = action_of(c)
    want = taxicab_golden(c)
    chain = chain_of(S, fields_of(c))
    one_shot = taxicab_one_shot(S, c['Links'])
    resident = taxicab_resident(chain)
    for got, how in ((one_shot, 'one-shot'), (resident, 'resident')):
        assert got.shape == want.shape and got.dtype == np.float64 and got[0, 0] == 1
        assert_relative(got, want, TOL, f'{case_id(c)} {how}')
    if c['kind'] == 'worldline' and c['W'] > 0:
        # the exact integer path: no result depends on how many origin units a workgroup takes
        try:
            for units in (2, 5):
                set_units(chain, units)
                assert np.array_equal(taxicab_resident(chain), resident), units
        finally:
            set_units(chain, 0)
    chain.close()


def exact_links(W, m, v):
    """W * Links.Worldline as integers: W m - delta(v)."""
    v = v[0]
    return np.stack([W * m[0] - (v - np.roll(v, 1, axis=1)), W * m[1] + (v - np.roll(v, 1, axis=0))]).astype(np.int64)


@pytest.mark.parametrize('N', [24, 96])
@pytest.mark.parametrize('kind,W,kappa', [('villain', 1, 0.5), ('worldline', 2, 0.5), ('worldline', float('inf'), 0.6)])
def test_taxicab_pair_on_device_generated_lattices(N, kind, W, kappa):
    """Not powers of two, several units and tiles, runs that wrap the boundary; a few hundred sweeps from a cold
    start keep the reweighting factors finite."""
    L = sv.Lattice2D(N)
    S = sv.Villain(L, kappa, W) if kind == 'villain' else sv.Worldline(L, kappa, W)
    chain = chain_of(S, sweeps=300, seed=N)
    chain.advance()
    got = taxicab_resident(chain)
    cfg = {k: np.array(x) for k, x in chain.download().items()}
    a, b = (2 * np.pi * kappa, -2 * np.pi * kappa * np.pi) if kind == 'villain' else (-1 / kappa, -1 / (2 * kappa))
    if kind == 'villain':
        links = O.Links.Villain(S, Form(cfg['phi'], degree=0, lattice=L), Form(cfg['n'], degree=1, lattice=L))
        want, M = taxicab_host(np.asarray(links), a, b, 1)
        rtol = 4 * abs(a) * 2 * N * EPS * M + 16 * EPS
    elif W < float('inf'):
        want, M = taxicab_host(exact_links(W, cfg['m'], cfg['v']), a, b, 0, W=float(W))
        rtol = TOL
    else:
        links = O.Links.Worldline(S, Form(cfg['m'], degree=1, lattice=L), Form(cfg['v'], degree=2, lattice=L))
        want, M = taxicab_host(np.asarray(links), a, b, 0)
        rtol = 4 * abs(a) * 2 * N * EPS * M + 16 * EPS
    assert M > 0 and np.isfinite(want).all() and np.isfinite(got).all()
    assert_relative(got, want, rtol, f'{kind} N={N} W={W} resident vs host restatement (M = {M})')
    if kind == 'worldline' and W < float('inf'):
        try:
            set_units(chain, 3)
            assert np.array_equal(taxicab_resident(chain), got)
        finally:
            set_units(chain, 0)
    else:
        assert_relative(taxicab_one_shot(S, links), want, rtol, f'{kind} N={N} W={W} one-shot vs host restatement')
    chain.close()


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
                O.Spin_Spin.resident(chain, path=path)
                O.Vortex_Vortex.resident(chain, path=path)
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
    L = sv.Lattice2D(8)
    S = sv.Villain(L, 0.5, 2) if kind == 'villain' else sv.Worldline(L, 0.5, 2)
    e = sv.Ensemble(S).generate(4, generator_for(S, seed=8))
    ss, vv = e.Spin_Spin, e.Vortex_Vortex
    assert ss.shape == (4, 8, 8) and vv.shape == (4, 8, 8)
    assert e.Spin_Spin is ss and e.Vortex_Vortex is vv
    for i in range(4):
        cfg = e.configuration[i]
        if kind == 'villain':
            links = O.Links.Villain(S, cfg['phi'], cfg['n'])
            want_ss, want_vv = O.Spin_Spin.Villain(S, cfg['phi']), O.Vortex_Vortex.Villain(S, links)
        else:
            links = O.Links.Worldline(S, cfg['m'], cfg['v'])
            want_ss, want_vv = O.Spin_Spin.Worldline(S, links), O.Vortex_Vortex.Worldline(S, cfg['v'])
        assert np.array_equal(ss[i], want_ss) and np.array_equal(vv[i], want_vv)


# ---- sizes no path serves ------------------------------------------------------------------------------------------

def test_unsupported_sizes_raise_not_implemented():
    f6 = np.ones((6, 6), dtype=complex)
    with pytest.raises(NotImplementedError, match='FFT'):
        O.correlation(sv.Lattice2D(6), f6, path=2)
    assert abs(O.correlation(sv.Lattice2D(6), f6, path=0) - 1).max() <= TOL  # (the direct sum serves it)
    S = sv.Villain(sv.Lattice2D(260), 0.5, 1)
    with pytest.raises(NotImplementedError, match='260'):
        O.Spin_Spin.Villain(S, np.zeros((1, 260, 260)))
    Sw = sv.Worldline(sv.Lattice2D(260), 0.5, 1)
    with pytest.raises(NotImplementedError, match='260'):
        O.Vortex_Vortex.Worldline(Sw, np.zeros((1, 260, 260), dtype=int))
