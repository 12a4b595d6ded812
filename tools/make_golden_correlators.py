"""Capture the reference's own two-point functions on equilibrated configurations (container-only; see
tools/refshim.py).  Run from the repo root:  python -m tools.make_golden_correlators

Writes tests/golden/correlators.npz: per case the action's parameters, the fields, and the outputs of the
reference's static methods on them:

  Links.Villain / Links.Worldline                     supervillain/observable/links.py:17-45
  Spin_Spin.Villain / Spin_Spin.Worldline             supervillain/observable/spin.py:28-42, :50-224
  Vortex_Vortex.Worldline / Vortex_Vortex.Villain     supervillain/observable/vortex.py:22-37, :63-189
  Spin_Spin_Normalized, SpinSusceptibility(Scaled), SpinCriticalMoment   spin.py:243-325
  Vortex_Vortex_Normalized, VortexSusceptibility(Scaled), VortexCriticalMoment   vortex.py:192-274

The configurations are equilibrated: SWEEPS NeighborhoodUpdate sweeps (Villain) or Sequentially(PlaquetteUpdate,
CoexactUpdate) steps (Worldline) of the reference's own generators from a seeded cold start, so that the taxicab
reweighting factors stay in the range a measurement meets (random fields give values beyond 1e177).  N <= 16: the
reference's taxicab index caches cost about 1 GB at N = 32.  N = 4 carries the direct pair only.
"""
import os

import numpy as np

from tools import refshim
from tools.make_golden import OUT, save

SWEEPS = 30
SIZES = (4, 5, 8, 16)
VILLAIN = ((1, 0.5), (2, 0.4))
WORLDLINE = ((1, 0.5), (2, 0.4), (float('inf'), 0.6))


def derived(sv, S, prefix, C):
    O = sv.observable
    norm = getattr(O, f'{prefix}_{prefix}_Normalized').default(S, C)
    chi = getattr(O, f'{prefix}Susceptibility').default(S, norm)
    return {f'{prefix}_{prefix}': np.asarray(C),
            f'{prefix}_{prefix}_Normalized': np.asarray(norm),
            f'{prefix}Susceptibility': np.asarray(chi),
            f'{prefix}SusceptibilityScaled': np.asarray(getattr(O, f'{prefix}SusceptibilityScaled').default(S, chi)),
            f'{prefix}CriticalMoment': np.asarray(getattr(O, f'{prefix}CriticalMoment').default(S, norm))}


def villain_case(sv, N, W, kappa, seed):
    O = sv.observable
    L = sv.lattice.Lattice2D(N)
    S = sv.action.Villain(L, kappa, W)
    G = sv.generator.villain.NeighborhoodUpdate(S)
    G.rng = np.random.default_rng(seed)
    cfg = S.configurations(1)[0]
    for _ in range(SWEEPS):
        cfg = G.step(cfg)
    phi, n = cfg['phi'], cfg['n']
    links = O.Links.Villain(S, phi, n)
    out = dict(kind='villain', N=N, W=W, kappa=kappa, seed=seed, taxicab=int(N > 4), phi=np.asarray(phi)[0].copy(),
               n=np.asarray(n).copy(), Links=np.asarray(links).copy())
    out |= derived(sv, S, 'Spin', O.Spin_Spin.Villain(S, phi))
    if N > 4:
        out |= derived(sv, S, 'Vortex', O.Vortex_Vortex.Villain(S, links))
    return out


def worldline_case(sv, N, W, kappa, seed):
    O = sv.observable
    L = sv.lattice.Lattice2D(N)
    S = sv.action.Worldline(L, kappa, W)
    P = sv.generator.worldline.PlaquetteUpdate(S)
    C = sv.generator.worldline.CoexactUpdate(S)
    P.rng = C.rng = np.random.default_rng(seed)
    cfg = S.configurations(1)[0]
    saved = np.random.get_state()
    np.random.seed(seed)  # PlaquetteUpdate's visit order comes from NumPy's global state (plaquette.py:63)
    for _ in range(SWEEPS):
        cfg = cfg | P.step(cfg)
        cfg = cfg | C.step(cfg)
    np.random.set_state(saved)
    m, v = cfg['m'], cfg['v']
    links = O.Links.Worldline(S, m, v)
    out = dict(kind='worldline', N=N, W=-1 if W == float('inf') else W, W_eff=S._W, kappa=kappa, seed=seed,
               taxicab=int(N > 4), m=np.asarray(m).copy(), v=np.asarray(v)[0].copy(), Links=np.asarray(links).copy())
    out |= derived(sv, S, 'Vortex', O.Vortex_Vortex.Worldline(S, v))
    if N > 4:
        out |= derived(sv, S, 'Spin', O.Spin_Spin.Worldline(S, links))
    return out


def main():
    sv = refshim.load()
    os.makedirs(OUT, exist_ok=True)
    cases, seed = [], 4100
    for N in SIZES:
        for W, kappa in VILLAIN:
            seed += 1
            cases.append(villain_case(sv, N, W, kappa, seed))
        for W, kappa in WORLDLINE:
            seed += 1
            cases.append(worldline_case(sv, N, W, kappa, seed))
    save('correlators.npz', cases)


if __name__ == '__main__':
    main()
