#!/usr/bin/env python
"""Time the device correlators (supervillain_amd/csrc/correlators.hip); one JSON line per case.

    python scripts/bench_correlators.py [--reps 5] [--out profiles/correlators.jsonl]

FFT path (Villain Spin_Spin of a resident configuration) at L = 1024 and 4096: hipEvent time of the six launches
(sv_ctx_set_timing) and wall time of the call (which ends with the download of the N*N complex128 result), the
bytes of the 8-pass estimate (8 streaming passes of 32 B per site) over the kernel time, and that rate as a fraction
of the copy-kernel ceiling sv_hbm_copy measures in the same run.  Taxicab kernel (Villain Vortex_Vortex and Worldline
Spin_Spin of resident configurations) at N = 64, 128, 256: the same two times and exps per second (V^2 exps).

A sanity condition, not a threshold: at L = 4096 the host route -- download the configuration, np.fft correlation --
must be slower than the device call.  If it is not, the script says so and exits 1.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import supervillain_amd as sv  # noqa: E402
from supervillain_amd import _native  # noqa: E402
from supervillain_amd import observable as O  # noqa: E402
from supervillain_amd.generator.combining import KeepEvery, Sequentially  # noqa: E402
from supervillain_amd.pipeline import DeviceChain, device_program  # noqa: E402


def chain_of(S, sweeps, seed):
    if isinstance(S, sv.Villain):
        G = sv.generator.villain.NeighborhoodUpdate(S, device=0)
        G.rng = np.random.default_rng(seed)
    else:
        P = sv.generator.worldline.PlaquetteUpdate(S, mode='checkerboard', device=0)
        C = sv.generator.worldline.CoexactUpdate(S, device=0)
        P.rng = C.rng = np.random.default_rng(seed)
        G = Sequentially([P, C])
    chain = DeviceChain(S, device_program(KeepEvery(sweeps, G)))
    chain.upload(S.configurations(1)[0])
    chain.advance()
    return chain


def timed(ctx, call, reps):
    """(median kernel ms, median wall ms, result) of `call` over reps timed runs after one warm-up."""
    lib = _native.lib()
    result = call()
    kernel, wall = [], []
    for _ in range(reps):
        ctx.check(lib.sv_ctx_set_timing(ctx.handle, 1), 'sv_ctx_set_timing')
        t0 = time.perf_counter()
        result = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, n = ctypes.c_double(), ctypes.c_int64()
        ctx.check(lib.sv_ctx_kernel_time(ctx.handle, ctypes.byref(ms), ctypes.byref(n)), 'sv_ctx_kernel_time')
        kernel.append(ms.value)
    ctx.check(lib.sv_ctx_set_timing(ctx.handle, 0), 'sv_ctx_set_timing')
    return float(np.median(kernel)), float(np.median(wall)), result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    lines, ok = [], True

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    ctx = _native.context(0)
    g = ctypes.c_double()
    ctx.check(_native.lib().sv_hbm_copy(ctx.handle, 1 << 30, 16, 20, ctypes.byref(g)), 'sv_hbm_copy')
    copy_GBps = g.value

    for N in (1024, 4096):
        S = sv.Villain(sv.Lattice2D(N), 0.5, 1)
        chain = chain_of(S, 5, N)
        kernel_ms, wall_ms, C = timed(chain.ctx, lambda: O.Spin_Spin.resident(chain, path=2), args.reps)
        est_bytes = 8 * 32 * N * N
        GBps = est_bytes / (kernel_ms * 1e-3) / 1e9
        d = dict(case='fft_spin_spin', N=N, kernel_ms=kernel_ms, wall_ms=wall_ms, estimate_bytes=est_bytes,
                 estimate_GBps=GBps, copy_ceiling_GBps=copy_GBps, fraction_of_copy_ceiling=GBps / copy_GBps)
        if N == 4096:
            t0 = time.perf_counter()
            f = np.exp(1j * chain.download()['phi'][0])
            F = np.fft.fft2(f, norm='ortho')
            H = np.fft.fft2(np.conj(F) * F, norm='ortho') / N
            d['host_download_npfft_ms'] = (time.perf_counter() - t0) * 1e3
            d['max_abs_device_minus_host'] = float(np.abs(C - H).max())
            d['host_slower_than_device'] = bool(d['host_download_npfft_ms'] > wall_ms)
            ok = ok and d['host_slower_than_device']
        emit(d)
        chain.close()

    for N in (64, 128, 256):
        for S, name, measure in ((sv.Villain(sv.Lattice2D(N), 0.5, 1), 'taxicab_villain_vortex_vortex', O.Vortex_Vortex),
                                 (sv.Worldline(sv.Lattice2D(N), 0.5, 2), 'taxicab_worldline_spin_spin_exact', O.Spin_Spin),
                                 (sv.Worldline(sv.Lattice2D(N), 0.6, float('inf')), 'taxicab_worldline_spin_spin_float',
                                  O.Spin_Spin)):
            chain = chain_of(S, 300, N)
            kernel_ms, wall_ms, out = timed(chain.ctx, lambda: measure.resident(chain), args.reps)
            exps = float(N) ** 4
            emit(dict(case=name, N=N, kernel_ms=kernel_ms, wall_ms=wall_ms, exps=exps,
                      exps_per_second=exps / (kernel_ms * 1e-3), finite=bool(np.isfinite(out).all())))
            chain.close()

    if args.out:
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    if not ok:
        print('sanity condition failed: host download + np.fft at L = 4096 was not slower than the device call',
              file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
