"""Two-point observables with the reference's names and call signatures (supervillain/observable/links.py,
spin.py, vortex.py), measured on the device.

The primary observables are classes of static methods, one per formulation, called as in the reference:

    Links.Villain(S, phi, n)            Links.Worldline(S, m, v)             host NumPy (links.py:17-45)
    Spin_Spin.Villain(S, phi)           Vortex_Vortex.Worldline(S, v)        one cross-correlation (sv_correlation)
    Spin_Spin.Worldline(S, Links)       Vortex_Vortex.Villain(S, Links)      taxicab reweighting (sv_taxicab_correlator)

`Spin_Spin.resident(chain)` and `Vortex_Vortex.resident(chain)` measure the configuration a
supervillain_amd.pipeline.DeviceChain holds, without a download.  The derived quantities (normalized correlators,
susceptibilities, critical moments) are host NumPy.  An Ensemble resolves the primary observables as attributes
(`ensemble.Spin_Spin`): an inline-measured column if there is one, else the measurement of every configuration, cached
on the ensemble (observable/observable.py:36-93).

There is no host fall-back: without libsvhip.so and a device the device-measured observables raise.
"""
import inspect

import numpy as np

from supervillain_amd import _native
from supervillain_amd.batch import Batch
from supervillain_amd.lattice import d, delta

registry = {}

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


class Observable:
    """A primary observable: measured configuration by configuration, resolved by Ensemble attribute access."""

    def __init_subclass__(cls):
        registry[cls.__name__] = cls


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


def _origin(S):
    return (0,) * S.Lattice.D


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
    cls = registry[name]
    if name in ensemble.__dict__:
        return ensemble.__dict__[name]
    fields = ensemble.configuration.fields
    if name in fields:
        return Batch.as_array(fields[name])
    kind = type(ensemble.Action).__name__
    method = getattr(cls, kind, None)
    if method is None:
        raise NotImplementedError(f'{name} not implemented for {kind}')
    args = [a for a in inspect.getfullargspec(method).args[1:] if a != 'path']
    columns = [getattr(ensemble, a) for a in args]
    values = [method(ensemble.Action, *row) for row in zip(*columns)]
    data = np.asarray(values)
    ensemble.__dict__[name] = Batch(data, dtype=data.dtype)
    return ensemble.__dict__[name]
