#!/usr/bin/env python
"""Time the packed action / winding two-point pass (supervillain_amd/csrc/correlators.hip); one JSON line per case.

    python scripts/bench_observables.py [--reps 5] [--out profiles/observables.jsonl]

On resident Villain and Worldline configurations at L = 1024 and 4096: hipEvent time of the launches
(sv_ctx_set_timing) and wall time of observable.action_winding (two N*N float64 downloads and the scalar sums
included), and in the same run Spin_Spin.resident of the Villain state (one transform pass of a field that needs no
neighbour) and the one-shot packed pass of host fields (the same six launches with a plain load, which separates what
the neighbour loads of the field formation add).

The condition the design sets, not a threshold: two autocorrelations cost two transform passes unpacked, so the
packed call's kernel time must be below twice the Spin_Spin kernel time of the same run at both sizes.  If it is not,
the script says so and exits 1.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import supervillain_amd as sv  # noqa: E402
from supervillain_amd import _native  # noqa: E402
from supervillain_amd import observable as O  # noqa: E402
from scripts.bench_correlators import chain_of, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    lines, ok = [], True

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    ctx = _native.context(0)
    for N in args.sizes:
        L = sv.Lattice2D(N)
        S = sv.Villain(L, 0.5, 1)
        chain = chain_of(S, 5, N)
        spin_ms, spin_wall, _ = timed(ctx, lambda: O.Spin_Spin.resident(chain, path=2), args.reps)
        emit(dict(case='fft_spin_spin', N=N, kernel_ms=spin_ms, wall_ms=spin_wall))
        kernel_ms, wall_ms, out = timed(ctx, lambda: O.action_winding(chain, path=2), args.reps)
        below = bool(kernel_ms < 2 * spin_ms)
        ok = ok and below
        emit(dict(case='packed_action_winding_villain', N=N, kernel_ms=kernel_ms, wall_ms=wall_ms,
                  ratio_to_spin_spin=kernel_ms / spin_ms, below_two_passes=below,
                  finite=bool(np.isfinite(out[0]).all() and np.isfinite(out[1]).all())))
        chain.close()

        r = np.random.default_rng(N)
        a, b = r.normal(size=(N, N)), r.normal(size=(N, N))
        plain_ms, plain_wall, _ = timed(ctx, lambda: O.correlation_real(L, a, b, path=2), args.reps)
        emit(dict(case='packed_one_shot_plain_load', N=N, kernel_ms=plain_ms, wall_ms=plain_wall,
                  villain_formation_share=(kernel_ms - plain_ms) / kernel_ms))

        Sw = sv.Worldline(L, 0.5, 2)
        chain = chain_of(Sw, 5, N)
        wl_ms, wl_wall, out = timed(ctx, lambda: O.action_winding(chain, path=2), args.reps)
        below = bool(wl_ms < 2 * spin_ms)
        ok = ok and below
        emit(dict(case='packed_action_winding_worldline_exact', N=N, kernel_ms=wl_ms, wall_ms=wl_wall,
                  ratio_to_spin_spin=wl_ms / spin_ms, below_two_passes=below,
                  worldline_formation_and_sums_share=(wl_ms - plain_ms) / wl_ms,
                  finite=bool(np.isfinite(out[0]).all() and np.isfinite(out[1]).all())))
        chain.close()

    if args.out:
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    if not ok:
        print('the packed pass was not below two Spin_Spin passes: the packing has failed', file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
