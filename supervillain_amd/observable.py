"""Two-point observables with the reference's names and call signatures (supervillain/observable/links.py,
spin.py, vortex.py), measured on the device.

The primary observables are classes of static methods, one per formulation, called as in the reference:

    Links.Villain(S, phi, n)            Links.Worldline(S, m, v)             host NumPy (links.py:17-45)
    Spin_Spin.Villain(S, phi)           Vortex_Vortex.Worldline(S, v)        one cross-correlation (sv_correlation)
    Spin_Spin.Worldline(S, Links)       Vortex_Vortex.Villain(S, Links)      taxicab reweighting (sv_taxicab_correlator)

    ActionTwoPoint.Villain/.Worldline(S, Links)                              one real autocorrelation
    Winding_Winding.Villain(S, n)       Winding_Winding.Worldline(S, Links)  (sv_correlation_real)
    ActionDensity, InternalEnergyDensity(Squared), WindingSquared, TorusWrapping, WrappingSquared   host NumPy

`action_winding(chain)` measures ActionTwoPoint and Winding_Winding of a resident configuration from one transform
pass of the packed fields, `scalars(chain)` its scalar observables from sums taken on the device.
`Spin_Spin.resident(chain)` and `Vortex_Vortex.resident(chain)` measure the configuration a
supervillain_amd.pipeline.DeviceChain holds, without a download.  The derived quantities (normalized correlators,
susceptibilities, critical moments) are host NumPy.  An Ensemble resolves the primary observables as attributes
(`ensemble.Spin_Spin`): an inline-measured column if there is one, else the measurement of every configuration, cached
on the ensemble (observable/observable.py:36-93).

There is no host fall-back: without libsvhip.so and a device the device-measured observables raise.
"""
import ctypes
import inspect

import numpy as np

from supervillain_amd import _native
from supervillain_amd._abi import SvWorldlineSums
from supervillain_amd.batch import Batch
from supervillain_amd.lattice import Form, d, delta

# rc -2 of a size no path serves: the library's message starts with this (include/supervillain_amd.h)
_NOT_IMPLEMENTED = 'not implemented'


def _check(ctx, rc, what):
    if rc == 0:
        return
    msg = _native.lib().sv_last_error(ctx.handle)
    text = msg.decode() if msg else str(rc)
    if rc == -2 and text.startswith(_NOT_IMPLEMENTED):
        raise NotImplementedError(f'{what}: {text}')
    raise _native.NativeError(f'{what} failed: {text}')


def _lattice_2d(S, what):
    L = S.Lattice
    if L.D != 2:
        raise NotImplementedError(f'{what} is measured on the device and only implemented for D=2.')
    return L


def correlation(L, f, path=0, device=None):
    """Lattice.correlation(f, f) (compact.py:465-...): C(r) = 1/V sum_x conj f(x) f(x - r) of one complex (N, N)
    field, on the device.  path: 0 auto, 1 direct sum, 2 FFT."""
    N = L.N
    f = np.ascontiguousarray(np.asarray(f, dtype=np.complex128).reshape(N, N))
    out = np.empty((N, N), dtype=np.complex128)
    ctx = _native.context(device)
    _check(ctx, _native.lib().sv_correlation(ctx.handle, N, _native.ptr(f), _native.ptr(out), int(path)),
           'sv_correlation')
    return out


def taxicab(L, links, a, b, dual, device=None):
    """out[dt, dx] = mean over origins of exp(a s + b (|dt| + |dx|)), s the signed sum of `links` over the fixed
    time-then-space path (dual: the path on the dual lattice), on the device."""
    N = L.N
    links = np.ascontiguousarray(np.asarray(links, dtype=np.float64).reshape(2, N, N))
    out = np.empty((N, N), dtype=np.float64)
    ctx = _native.context(device)
    _check(ctx, _native.lib().sv_taxicab_correlator(ctx.handle, N, _native.ptr(links), float(a), float(b), int(dual),
                                                    _native.ptr(out)), 'sv_taxicab_correlator')
    return out


def correlation_real(L, a, b=None, path=0, device=None):
    """Lattice.correlation(a, a) of a real (N, N) field, and with b also Lattice.correlation(b, b), both from one
    transform pass of a + i b on the device (sv_correlation_real).  Real float64 (N, N); (C_aa, C_bb) with b.
    path: 0 auto, 1 direct sum, 2 FFT."""
    N = L.N
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(N, N))
    out_aa = np.empty((N, N), dtype=np.float64)
    if b is not None:
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(N, N))
        out_bb = np.empty((N, N), dtype=np.float64)
    ctx = _native.context(device)
    null = ctypes.c_void_p(None)
    _check(ctx, _native.lib().sv_correlation_real(ctx.handle, N, _native.ptr(a), null if b is None else _native.ptr(b),
                                                  _native.ptr(out_aa), null if b is None else _native.ptr(out_bb),
                                                  int(path)), 'sv_correlation_real')
    return out_aa if b is None else (out_aa, out_bb)


def _form(x, degree, L):
    return x if isinstance(x, Form) else Form(np.asarray(x), degree=degree, lattice=L)


# every primary observable by name: what an Ensemble resolves as an attribute
primary = {}


class Observable:
    """A primary observable: measured configuration by configuration, resolved by Ensemble attribute access."""

    def __init_subclass__(cls):
        primary[cls.__name__] = cls


class DerivedQuantity:
    """A function of expectation values (host NumPy); `default(S, ...)` as in the reference."""


class Links(Observable):
    """The gauge-invariant link variables of either formulation (links.py:5-45)."""

    @staticmethod
    def Villain(S, phi, n):
        return d(phi) - 2 * np.pi * n

    @staticmethod
    def Worldline(S, m, v):
        return m - delta(v) / S._W


class Spin_Spin(Observable):
    """Spin_Spin[dx] = 1/V sum_x S(x, x - dx) (spin.py:5-241)."""

    @staticmethod
    def Villain(S, phi, path=0):
        """<exp(i (phi_x - phi_y))>: the correlation of exp(i phi) (spin.py:28-42)."""
        L = _lattice_2d(S, 'The Villain Spin_Spin')
        return correlation(L, np.exp(1.j * np.asarray(phi)[0]), path)

    @staticmethod
    def Worldline(S, Links):
        """The taxicab reweighting exp(-1/(2 kappa) (2 P.m + |P|)) averaged over origins (spin.py:50-224)."""
        if S.Lattice.D != 2:
            raise NotImplementedError(
                'The Worldline Spin_Spin measurement traces a taxicab path on the lattice and is '
                'only implemented for D=2.')
        return taxicab(S.Lattice, Links, -1 / S.kappa, -1 / (2 * S.kappa), 0)

    @staticmethod
    def resident(chain, path=0):
        """Spin_Spin of the configuration a DeviceChain holds (sv_villain_spin_spin / sv_worldline_spin_spin)."""
        S, N, lib = chain.Action, chain.N, _native.lib()
        if chain.kind == 'villain':
            out = np.empty((N, N), dtype=np.complex128)
            _check(chain.ctx, lib.sv_villain_spin_spin(chain.handle, _native.ptr(out), int(path)), 'sv_villain_spin_spin')
        else:
            out = np.empty((N, N), dtype=np.float64)
            _check(chain.ctx, lib.sv_worldline_spin_spin(chain.handle, float(S.kappa), float(S._W), _native.ptr(out)),
                   'sv_worldline_spin_spin')
        return out

    @staticmethod
    def CriticalScalingDimension(S):
        """W^2 / 8, or 1 / (pi kappa) at W = infinity (spin.py:226-241)."""
        W = S.W
        if W < float('inf'):
            return W ** 2 / 8
        return 1 / S.kappa / np.pi


class Vortex_Vortex(Observable):
    """Vortex_Vortex[dx] = 1/V sum_x V(x, x - dx) (vortex.py:6-189)."""

    @staticmethod
    def Worldline(S, v, path=0):
        """<exp(2 pi i (v_x - v_y) / W)>: the correlation of exp(2 pi i v / W) (vortex.py:22-37)."""
        L = S.Lattice
        if L.D < 2:
            raise NotImplementedError('Vortex observables require D >= 2; there are no plaquettes for D < 2.')
        _lattice_2d(S, 'The Worldline Vortex_Vortex')
        return correlation(L, np.exp(2j * np.pi * np.asarray(v)[0] / S._W), path)

    @staticmethod
    def Villain(S, Links):
        """The taxicab reweighting on the dual lattice, exp(2 pi kappa (P.Links - pi |P|)), averaged over origins
        (vortex.py:63-189)."""
        if S.Lattice.D != 2:
            raise NotImplementedError(
                'The Villain Vortex_Vortex measurement traces a taxicab path on the dual lattice '
                'and is only implemented for D=2.')
        return taxicab(S.Lattice, Links, 2 * np.pi * S.kappa, -2 * np.pi * S.kappa * np.pi, 1)

    @staticmethod
    def resident(chain, path=0):
        """Vortex_Vortex of the configuration a DeviceChain holds (sv_worldline_vortex_vortex /
        sv_villain_vortex_vortex)."""
        S, N, lib = chain.Action, chain.N, _native.lib()
        if chain.kind == 'villain':
            out = np.empty((N, N), dtype=np.float64)
            _check(chain.ctx, lib.sv_villain_vortex_vortex(chain.handle, float(S.kappa), _native.ptr(out)),
                   'sv_villain_vortex_vortex')
        else:
            out = np.empty((N, N), dtype=np.complex128)
            _check(chain.ctx, lib.sv_worldline_vortex_vortex(chain.handle, float(S._W), _native.ptr(out), int(path)),
                   'sv_worldline_vortex_vortex')
        return out

    @staticmethod
    def CriticalScalingDimension(S):
        """2 / W^2, or 4 pi kappa at W = infinity (vortex.py:39-57)."""
        W = S.W
        if W < float('inf'):
            return 2 / W ** 2
        return 4 * np.pi * S.kappa


# The link, spin and vortex observables (correlators.hip's two pairs), under the name this dict has always had; the
# action and winding observables below are in `primary` only.
registry = dict(primary)


def _origin(S):
    return (0,) * S.Lattice.D


def _links_squared(Links):
    return (np.asarray(Links) ** 2).sum()


def _villain_action(S, phi, n):
    L = S.Lattice
    return S(_form(phi, 0, L), _form(n, 1, L))


class ActionDensity(Observable):
    """<kappa d/dkappa S> / sites (action.py:4-47).  Host NumPy."""

    @staticmethod
    def Villain(S, phi, n):
        return _villain_action(S, phi, n) / S.Lattice.cells_of_degree[0]

    @staticmethod
    def Worldline(S, Links):
        L = S.Lattice
        return (L.links / 2 - 0.5 / S.kappa * _links_squared(Links)) / L.sites


class InternalEnergyDensity(Observable):
    """<d/dkappa S> / sites (energy.py:4-46).  Host NumPy."""

    @staticmethod
    def Villain(S, phi, n):
        return _villain_action(S, phi, n) / (S.Lattice.cells_of_degree[0] * S.kappa)

    @staticmethod
    def Worldline(S, Links):
        L = S.Lattice
        return (L.links / 2 - 0.5 / S.kappa * _links_squared(Links)) / (L.sites * S.kappa)


class InternalEnergyDensitySquared(Observable):
    """<(d/dkappa S)^2 - d^2/dkappa^2 S> / sites^2 (energy.py:48-102).  Host NumPy."""

    @staticmethod
    def Villain(S, phi, n):
        return (_villain_action(S, phi, n) / (S.Lattice.cells_of_degree[0] * S.kappa)) ** 2

    @staticmethod
    def Worldline(S, Links):
        L = S.Lattice
        l2 = _links_squared(Links)
        partial_kappa_S = (L.links / 2 - 0.5 / S.kappa * l2) / S.kappa
        partial_2_kappa_S = (l2 / S.kappa - L.links / 2) / S.kappa ** 2
        return (partial_kappa_S ** 2 - partial_2_kappa_S) / L.sites ** 2


def _needs_plaquettes(S):
    if S.Lattice.D < 2:
        raise NotImplementedError('Winding observables require D >= 2; there are no plaquettes for D < 2.')


class WindingSquared(Observable):
    """The plaquette winding number squared, averaged over the lattice (winding.py:8-52).  Host NumPy."""

    @staticmethod
    def Villain(S, n):
        _needs_plaquettes(S)
        return np.mean(np.asarray(d(_form(n, 1, S.Lattice))) ** 2)

    @staticmethod
    def Worldline(S, Links):
        _needs_plaquettes(S)
        dl = np.asarray(d(_form(Links, 1, S.Lattice)))
        return 1 / (np.pi ** 2 * S.kappa) - np.mean(dl ** 2) / (2 * np.pi * S.kappa) ** 2


class TorusWrapping(Observable):
    """The integers that wrap the torus, one per direction (wrapping.py:4-39).  Host NumPy."""

    @staticmethod
    def Villain(S, phi, n):
        n = np.asarray(n)
        return n.sum(axis=tuple(range(1, n.ndim)))

    @staticmethod
    def Worldline(S, m):
        m = np.asarray(m)
        return m.sum(axis=tuple(range(1, m.ndim))) / S.Lattice.N


class WrappingSquared(Observable):
    """sum_mu TorusWrapping_mu^2 (wrapping.py:41-59)."""

    @staticmethod
    def default(S, TorusWrapping):
        return (np.asarray(TorusWrapping) ** 2).sum()


class ActionTwoPoint(Observable):
    """ActionTwoPoint[dx] = 1/V sum_x S^2(x, x - dx), the translation-averaged two-point function of the local
    action derivative with its contact terms (action.py:49-152).

    Real float64 (N, N).  The reference returns complex128 whose imaginary part is round-off (its correlation goes
    through a complex FFT); here the correlation of a real field is real by construction."""

    @staticmethod
    def Villain(S, Links, path=0):
        L = _lattice_2d(S, 'ActionTwoPoint')
        density = 0.5 * S.kappa * (np.asarray(Links) ** 2).sum(axis=0)
        result = correlation_real(L, density, path=path)
        result[_origin(S)] -= density.mean()
        return result

    @staticmethod
    def Worldline(S, Links, path=0):
        L = _lattice_2d(S, 'ActionTwoPoint')
        m_squared = (np.asarray(Links) ** 2).sum(axis=0)
        derivative = 1 - 0.5 / S.kappa * m_squared
        result = correlation_real(L, derivative, path=path)
        result[_origin(S)] -= (m_squared / 2 / S.kappa).mean()
        return result

    @staticmethod
    def resident(chain, path=0):
        """ActionTwoPoint of the configuration a DeviceChain holds (sv_*_action_winding)."""
        return _action_winding(chain, path, True, False)[0]


class Winding_Winding(Observable):
    """Winding_Winding[dp] = 1/V sum_p W(p, p - dp), the correlations of the plaquette winding number
    (winding.py:54-202).  Winding_Winding[origin] equals WindingSquared configuration by configuration.

    Real float64 (N, N); the reference returns complex128 whose imaginary part is round-off."""

    _stencil = {}

    @staticmethod
    def contact(L):
        """d(delta(unit source)) at the origin plaquette, the J-independent contact term (winding.py:184-200)."""
        key = (L.D, L.N)
        if key not in Winding_Winding._stencil:
            source = L.form(2)
            source[0][(0,) * L.D] = 1.
            Winding_Winding._stencil[key] = np.asarray(d(delta(source)))[0].copy()
        return Winding_Winding._stencil[key]

    @staticmethod
    def Villain(S, n, path=0):
        _needs_plaquettes(S)
        L = _lattice_2d(S, 'Winding_Winding')
        return correlation_real(L, np.asarray(d(_form(n, 1, L)))[0], path=path)

    @staticmethod
    def Worldline(S, Links, path=0):
        _needs_plaquettes(S)
        L = _lattice_2d(S, 'Winding_Winding')
        dm = np.asarray(d(_form(Links, 1, L)))[0]
        return (S.kappa * Winding_Winding.contact(L) - correlation_real(L, dm, path=path)) / (2 * np.pi * S.kappa) ** 2

    @staticmethod
    def resident(chain, path=0):
        """Winding_Winding of the configuration a DeviceChain holds (sv_*_action_winding)."""
        return _action_winding(chain, path, False, True)[1]


def sums(chain):
    """The raw sums of the configuration a DeviceChain holds, as the device computes them.  Villain: {'S', 'dn2',
    'n0', 'n1'} (sv_villain_observables).  Worldline: the fields of sv_worldline_sums (sv_worldline_observables)."""
    return _sums_dict(chain, _measure_sums(chain))


def _measure_sums(chain):
    S, lib = chain.Action, _native.lib()
    if chain.kind == 'villain':
        out = np.zeros(4)
        chain.ctx.check(lib.sv_villain_observables(chain.handle, float(S.kappa), _native.ptr(out)),
                        'sv_villain_observables')
        return out
    out = SvWorldlineSums()
    _check(chain.ctx, lib.sv_worldline_observables(chain.handle, float(S.kappa), float(S._W), ctypes.byref(out)),
           'sv_worldline_observables')
    return out


def _sums_dict(chain, raw):
    if chain.kind == 'villain':
        return {'S': float(raw[0]), 'dn2': int(round(raw[1])), 'n0': int(round(raw[2])), 'n1': int(round(raw[3]))}
    return {name: getattr(raw, name) for name, _ in SvWorldlineSums._fields_}


def _scalars_dict(chain, raw):
    """The scalar observables from the device sums, in the reference's expressions (action.py:25-47, energy.py:25-102,
    winding.py:30-52, wrapping.py:17-39)."""
    S = chain.Action
    L, kappa = S.Lattice, S.kappa
    if chain.kind == 'villain':
        action, V = float(raw[0]), L.cells_of_degree[0]
        return {'ActionDensity': action / V,
                'InternalEnergyDensity': action / (V * kappa),
                'InternalEnergyDensitySquared': (action / (V * kappa)) ** 2,
                'WindingSquared': raw[1] / L.cells_of_degree[2],
                'TorusWrapping': np.array([int(round(raw[2])), int(round(raw[3]))], dtype=np.int64)}
    l2 = raw.links_squared
    partial_kappa_S = (L.links / 2 - 0.5 / kappa * l2) / kappa
    partial_2_kappa_S = (l2 / kappa - L.links / 2) / kappa ** 2
    return {'ActionDensity': (L.links / 2 - 0.5 / kappa * l2) / L.sites,
            'InternalEnergyDensity': (L.links / 2 - 0.5 / kappa * l2) / (L.sites * kappa),
            'InternalEnergyDensitySquared': (partial_kappa_S ** 2 - partial_2_kappa_S) / L.sites ** 2,
            'WindingSquared': 1 / (np.pi ** 2 * kappa) - raw.curl_squared / L.cells_of_degree[2] / (2 * np.pi * kappa) ** 2,
            'TorusWrapping': np.array([raw.m0, raw.m1], dtype=np.int64) / L.N}


def scalars(chain):
    """ActionDensity, InternalEnergyDensity, InternalEnergyDensitySquared, WindingSquared and TorusWrapping of the
    configuration a DeviceChain holds, either formulation, from sums taken on the device (no download)."""
    return _scalars_dict(chain, _measure_sums(chain))


def _action_winding(chain, path, want_action, want_winding):
    S, N, lib = chain.Action, chain.N, _native.lib()
    action = np.empty((N, N), dtype=np.float64) if want_action else None
    winding = np.empty((N, N), dtype=np.float64) if want_winding else None
    pa = ctypes.c_void_p(None) if action is None else _native.ptr(action)
    pw = ctypes.c_void_p(None) if winding is None else _native.ptr(winding)
    if chain.kind == 'villain':
        raw = np.zeros(4)
        _check(chain.ctx, lib.sv_villain_action_winding(chain.handle, float(S.kappa), pa, pw, _native.ptr(raw), int(path)),
               'sv_villain_action_winding')
    else:
        raw = SvWorldlineSums()
        _check(chain.ctx, lib.sv_worldline_action_winding(chain.handle, float(S.kappa), float(S._W), pa, pw,
                                                          ctypes.byref(raw), int(path)), 'sv_worldline_action_winding')
    return action, winding, _scalars_dict(chain, raw)


def action_winding(chain, path=0):
    """(ActionTwoPoint, Winding_Winding, scalars) of the configuration a DeviceChain holds: the two correlators from
    one transform pass of the packed fields (sv_villain_action_winding / sv_worldline_action_winding), `scalars` as
    scalars(chain) gives them."""
    return _action_winding(chain, path, True, True)


class InternalEnergyDensityVariance(DerivedQuantity):
    """<U^2 / sites^2> - <U / sites>^2 (energy.py:104-118)."""

    @staticmethod
    def default(S, InternalEnergyDensitySquared, InternalEnergyDensity):
        return InternalEnergyDensitySquared - InternalEnergyDensity ** 2


class SpecificHeatCapacity(DerivedQuantity):
    """kappa^2 sites InternalEnergyDensityVariance (energy.py:120-136)."""

    @staticmethod
    def default(S, InternalEnergyDensityVariance):
        return InternalEnergyDensityVariance * S.Lattice.sites * S.kappa ** 2


class Action_Action(DerivedQuantity):
    """ActionTwoPoint - <ActionDensity>^2 (action.py:154-215)."""

    @staticmethod
    def default(S, ActionTwoPoint, ActionDensity):
        return ActionTwoPoint - ActionDensity ** 2


def _r_squared(L):
    return np.sum(L.coords ** 2, axis=0)


class Spin_Spin_Normalized(DerivedQuantity):
    """Spin_Spin / Spin_Spin[origin] (spin.py:243-263)."""

    @staticmethod
    def default(S, Spin_Spin):
        return Spin_Spin / Spin_Spin[_origin(S)]


class SpinSusceptibility(DerivedQuantity):
    """The sum over the lattice of the normalized correlator (spin.py:265-276)."""

    @staticmethod
    def default(S, Spin_Spin_Normalized):
        return np.sum(Spin_Spin_Normalized.real)


class SpinSusceptibilityScaled(SpinSusceptibility):
    """chi_S / N^(D - 2 Delta_S) (spin.py:278-304)."""

    @staticmethod
    def default(S, SpinSusceptibility):
        L = S.Lattice
        return SpinSusceptibility / L.N ** (L.D - 2 * Spin_Spin.CriticalScalingDimension(S))


class SpinCriticalMoment(DerivedQuantity):
    """1/V sum_r r^(2 Delta_S) S(r) (spin.py:306-325)."""

    @staticmethod
    def default(S, Spin_Spin_Normalized):
        L = S.Lattice
        return np.sum(_r_squared(L) ** Spin_Spin.CriticalScalingDimension(S) * Spin_Spin_Normalized.real) / L.sites


class Vortex_Vortex_Normalized(DerivedQuantity):
    """Vortex_Vortex / Vortex_Vortex[origin] (vortex.py:192-211)."""

    @staticmethod
    def default(S, Vortex_Vortex):
        return Vortex_Vortex / Vortex_Vortex[_origin(S)]


class VortexSusceptibility(DerivedQuantity):
    """The sum over the lattice of the normalized correlator (vortex.py:213-224)."""

    @staticmethod
    def default(S, Vortex_Vortex_Normalized):
        return np.sum(Vortex_Vortex_Normalized.real)


class VortexSusceptibilityScaled(VortexSusceptibility):
    """chi_V / N^(D - 2 Delta_V) (vortex.py:227-254)."""

    @staticmethod
    def default(S, VortexSusceptibility):
        L = S.Lattice
        return VortexSusceptibility / L.N ** (L.D - 2 * Vortex_Vortex.CriticalScalingDimension(S))


class VortexCriticalMoment(DerivedQuantity):
    """1/V sum_r r^(2 Delta_V) V(r) (vortex.py:256-274)."""

    @staticmethod
    def default(S, Vortex_Vortex_Normalized):
        L = S.Lattice
        return np.sum(_r_squared(L) ** Vortex_Vortex.CriticalScalingDimension(S) * Vortex_Vortex_Normalized.real) / L.sites


def measure(ensemble, name):
    """The observable `name` of every configuration of an ensemble (observable/observable.py:36-93): the cached
    result, else an inline-measured column, else the action's measurement applied to each configuration, its
    arguments (fields or other observables) looked up by name on the ensemble.  Cached on the ensemble."""
    cls = primary[name]
    if name in ensemble.__dict__:
        return ensemble.__dict__[name]
    fields = ensemble.configuration.fields
    if name in fields:
        return Batch.as_array(fields[name])
    kind = type(ensemble.Action).__name__
    # the formulation's own measurement, else the one `default` gives from its arguments (observable.py:60-75)
    method = getattr(cls, kind, None) or getattr(cls, 'default', None)
    if method is None:
        raise NotImplementedError(f'{name} not implemented for {kind}')
    args = [a for a in inspect.getfullargspec(method).args[1:] if a != 'path']
    columns = [getattr(ensemble, a) for a in args]
    values = [method(ensemble.Action, *row) for row in zip(*columns)]
    data = np.asarray(values)
    ensemble.__dict__[name] = Batch(data, dtype=data.dtype)
    return ensemble.__dict__[name]
