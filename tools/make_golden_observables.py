"""Capture the reference's own inline-observable values along seeded Villain chains (container-only; see
tools/refshim.py).  Run from the repo root:  python -m tools.make_golden_observables [chains] [single]
(no argument: both files; `single` writes tests/golden/observables.npz alone, see single_configurations below)

Writes tests/golden/villain_observables.npz: per chain the inputs (N, kappa, W, seed, hot-start seed), the
bit-generator states before and after, and after EVERY sweep of NeighborhoodUpdate.step the four scalars the
reference measures on a Villain configuration:

  ActionDensity.Villain          supervillain/observable/action.py:25-31    S(phi, n) / |sites|
  InternalEnergyDensity.Villain  supervillain/observable/energy.py:25-30    S(phi, n) / (|sites| kappa)
  WindingSquared.Villain         supervillain/observable/winding.py:30-37   mean(d(n)**2)
  TorusWrapping.Villain          supervillain/observable/wrapping.py:17-25  n.sum over sites, per direction

computed by those static methods themselves on the reference's own chain (neighborhood.py:59-137).  Chains of one
(N, kappa, W) share a group so that a replica batch (one kappa and W per batch) can run them together.
"""
import os
import sys

import numpy as np

from tools import refshim
from tools.make_golden import OUT, rng_state, save

# (group, N, kappa, W, sweeps, seed, hot_seed or None)
CHAINS = [
    ('n8w1', 8, 0.5, 1, 6, 21, None), ('n8w1', 8, 0.5, 1, 6, 22, 221),
    ('n8w2', 8, 0.3, 2, 6, 23, 231), ('n8w2', 8, 0.3, 2, 6, 24, 241),
    ('n16w1', 16, 0.4, 1, 5, 25, 251), ('n16w1', 16, 0.4, 1, 5, 26, 261), ('n16w1', 16, 0.4, 1, 5, 27, None),
    ('n16w2', 16, 0.5, 2, 5, 28, 281), ('n16w2', 16, 0.5, 2, 5, 29, 291),
    ('n128w2', 128, 0.5, 2, 4, 30, 301), ('n128w2', 128, 0.5, 2, 4, 31, 311), ('n128w2', 128, 0.5, 2, 4, 32, None),
    ('n128w1', 128, 0.5, 1, 4, 33, 331), ('n128w1', 128, 0.5, 1, 4, 34, 341),
]


def hot_start(N, W, hot_seed):
    """The hot start of tools/make_golden.villain_chain (phi uniform in [-pi, pi), n in W * {-2..2})."""
    if hot_seed is None:
        return np.zeros((N, N)), np.zeros((2, N, N), dtype=np.int64)
    r = np.random.default_rng(hot_seed)
    return r.uniform(-np.pi, np.pi, (1, N, N))[0], (W * r.integers(-2, 3, (2, N, N))).astype(np.int64)


def chain(sv, group, N, kappa, W, sweeps, seed, hot_seed):
    from supervillain.observable.action import ActionDensity
    from supervillain.observable.energy import InternalEnergyDensity
    from supervillain.observable.winding import WindingSquared
    from supervillain.observable.wrapping import TorusWrapping
    L = sv.lattice.Lattice2D(N)
    S = sv.action.Villain(L, kappa, W)
    G = sv.generator.villain.NeighborhoodUpdate(S)
    G.rng = np.random.default_rng(seed)
    phi0, n0 = hot_start(N, W, hot_seed)
    cfg = {'phi': sv.lattice.Form(phi0[None].copy(), degree=0, lattice=L),
           'n': sv.lattice.Form(n0.copy(), degree=1, lattice=L)}
    rng0 = rng_state(G.rng)
    ad, ie, w2, tw = [], [], [], []
    for _ in range(sweeps):
        cfg = G.step(cfg)
        phi, n = cfg['phi'], cfg['n']
        ad.append(float(ActionDensity.Villain(S, phi, n)))
        ie.append(float(InternalEnergyDensity.Villain(S, phi, n)))
        w2.append(float(WindingSquared.Villain(S, n)))
        tw.append(np.asarray(TorusWrapping.Villain(S, phi, n), dtype=np.int64))
    return dict(group=group, N=N, kappa=kappa, W=W, sweeps=sweeps, seed=seed,
                hot_seed=-1 if hot_seed is None else hot_seed, rng0=rng0, rng1=rng_state(G.rng),
                ActionDensity=np.array(ad), InternalEnergyDensity=np.array(ie), WindingSquared=np.array(w2),
                TorusWrapping=np.array(tw, dtype=np.int64))


# ---- tests/golden/observables.npz: every action, energy, winding and wrapping observable on single configurations ----
#
# Per case the fields, Links and the reference's output of every primary observable of
# supervillain/observable/{action,energy,winding,wrapping}.py and, evaluated on that one configuration's values, the
# derived quantities InternalEnergyDensityVariance, SpecificHeatCapacity and Action_Action.  These are pure
# measurements, so the Villain fields need not be equilibrated: phi uniform in (-pi, pi) and n integer in [-2, 2] from
# a recorded seed, advanced until at least V/4 plaquettes of d(n) are nonzero and both torus wrappings are nonzero.
# Worldline: the equilibrated (m, v) of correlators.npz, and per N one random (m, v) with both wrappings nonzero.
SIZES = (2, 3, 4, 5, 8, 16)
VILLAIN = ((1, 0.5), (2, 0.4))
RANDOM_WORLDLINE = (2, 0.5)


def measured(sv, S, kind, fields, links):
    """The reference's outputs on one configuration; None when it does not accept the lattice."""
    O = sv.observable
    if kind == 'villain':
        phi, n = fields
        scalar_args = {'ActionDensity': (phi, n), 'InternalEnergyDensity': (phi, n),
                       'InternalEnergyDensitySquared': (phi, n), 'WindingSquared': (n,), 'TorusWrapping': (phi, n),
                       'ActionTwoPoint': (links,), 'Winding_Winding': (n,)}
    else:
        m, v = fields
        scalar_args = {'ActionDensity': (links,), 'InternalEnergyDensity': (links,),
                       'InternalEnergyDensitySquared': (links,), 'WindingSquared': (links,), 'TorusWrapping': (m,),
                       'ActionTwoPoint': (links,), 'Winding_Winding': (links,)}
    method = 'Villain' if kind == 'villain' else 'Worldline'
    out = {name: np.asarray(getattr(getattr(O, name), method)(S, *args)) for name, args in scalar_args.items()}
    out['WrappingSquared'] = np.asarray(O.WrappingSquared.default(S, out['TorusWrapping']))
    variance = O.InternalEnergyDensityVariance.default(S, out['InternalEnergyDensitySquared'],
                                                       out['InternalEnergyDensity'])
    out['InternalEnergyDensityVariance'] = np.asarray(variance)
    out['SpecificHeatCapacity'] = np.asarray(O.SpecificHeatCapacity.default(S, variance))
    out['Action_Action'] = np.asarray(O.Action_Action.default(S, out['ActionTwoPoint'], out['ActionDensity']))
    return out


def villain_single(sv, N, W, kappa, seed):
    O = sv.observable
    L = sv.lattice.Lattice2D(N)
    S = sv.action.Villain(L, kappa, W)
    while True:
        r = np.random.default_rng(seed)
        phi = sv.lattice.Form(r.uniform(-np.pi, np.pi, (1, N, N)), degree=0, lattice=L)
        n = sv.lattice.Form(r.integers(-2, 3, (2, N, N)).astype(np.int64), degree=1, lattice=L)
        wrapping = np.asarray(O.TorusWrapping.Villain(S, phi, n))
        if np.count_nonzero(np.asarray(sv.lattice.d(n))) >= N * N / 4 and (wrapping != 0).all():
            break
        seed += 1000
    links = O.Links.Villain(S, phi, n)
    return dict(kind='villain', N=N, W=W, kappa=kappa, seed=seed, phi=np.asarray(phi)[0].copy(), n=np.asarray(n).copy(),
                Links=np.asarray(links).copy()) | measured(sv, S, 'villain', (phi, n), links)


def worldline_single(sv, N, W, kappa, m, v, seed, source):
    O = sv.observable
    L = sv.lattice.Lattice2D(N)
    S = sv.action.Worldline(L, kappa, W)
    m = sv.lattice.Form(np.asarray(m), degree=1, lattice=L)
    v = sv.lattice.Form(np.asarray(v)[None], degree=2, lattice=L)
    links = O.Links.Worldline(S, m, v)
    return dict(kind='worldline', N=N, W=-1 if W == float('inf') else W, W_eff=S._W, kappa=kappa, seed=seed,
                source=source, m=np.asarray(m).copy(), v=np.asarray(v)[0].copy(),
                Links=np.asarray(links).copy()) | measured(sv, S, 'worldline', (m, v), links)


def worldline_random(sv, N, seed):
    W, kappa = RANDOM_WORLDLINE
    while True:
        r = np.random.default_rng(seed)
        m = r.integers(-2, 3, (2, N, N)).astype(np.int64)
        v = r.integers(-3, 4, (N, N)).astype(np.int64)
        if (m.sum(axis=(1, 2)) != 0).all():
            break
        seed += 1000
    return worldline_single(sv, N, W, kappa, m, v, seed, 'random')


def load_cases(name):
    z = np.load(os.path.join(OUT, name), allow_pickle=False)
    return [{k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(f'{i}/')} for i in range(int(z['count']))]


def single_configurations(sv):
    cases, seed = [], 5200
    for N in SIZES:
        made = []
        try:
            for W, kappa in VILLAIN:
                seed += 1
                made.append(villain_single(sv, N, W, kappa, seed))
            seed += 1
            made.append(worldline_random(sv, N, seed))
        except Exception as e:  # (N = 2 is kept only if the reference accepts it)
            if N != 2:
                raise
            print(f'N = {N}: the reference refuses it ({type(e).__name__}: {e}); left out')
            continue
        cases += made
    for c in load_cases('correlators.npz'):
        if str(c['kind']) == 'worldline':
            W = float('inf') if int(c['W']) < 0 else int(c['W'])
            cases.append(worldline_single(sv, int(c['N']), W, float(c['kappa']), c['m'], c['v'], int(c['seed']),
                                          'correlators.npz'))
    return cases


def main():
    sv = refshim.load()
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ['chains', 'single']
    if 'chains' in which:
        save('villain_observables.npz', [chain(sv, *c) for c in CHAINS])
    if 'single' in which:
        save('observables.npz', single_configurations(sv))


if __name__ == '__main__':
    main()
