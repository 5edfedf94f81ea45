"""The double-double (option_mpmath) chain beside the float64 fused chain, and the 'ray_wave' mode
with option_mpmath=True on the device:

    python scripts/bench_dd.py [--n 1001] [--reps 20] [--mode-size 65] [--out bench_out/bench_dd.json]

* rays/s of akb_trace_chain_dd_f64 and of akb_trace_chain_f64 for the same launch (the AKB's four
  mirrors of tests/golden/akb_geometry.json on an n x n grid, last hit + exit direction + OPL rows),
  timed with device events over `reps` launches after a warm-up, and their ratio;
* wall time of driver.plot_result_ray_wave(option_mpmath=True) and of the float64 call at
  mode-size^2 (median of seven after a warm-up).

The reference's own mpmath branch for the same 65^2 call is a CPU measurement (DESIGN.md quotes
it); nothing here reads the reference.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_driver import best_params  # noqa: E402


def chain_rate(g, n, precision, reps):
    from akbraytracing_amd.trace import ChainLaunch
    dev = torch.device("cuda", 0)
    tan_h = torch.from_numpy(np.tan(g.angle_h.table(n))).to(dev)
    tan_v = torch.from_numpy(np.tan(g.angle_v.table(n))).to(dev)
    c = ChainLaunch(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, want=("last_hit", "dir_out", "opl"),
                    precision=precision)
    for _ in range(3):
        c.launch()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for k in range(reps):
        c.launch(reset_flags=False)
        ev[k + 1].record()
    torch.cuda.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]
    med = float(np.median(ms))
    return dict(ms_median=med, ms_min=float(min(ms)), rays_per_s=n * n / (med * 1e-3), flags=int(c.res.flags.item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1001)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode-size", type=int, default=65)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from akbraytracing_amd.driver import plot_result_ray_wave
    from akbraytracing_amd.wavefront import SystemGeometry
    g = SystemGeometry.load(os.path.join(ROOT, "tests", "golden", "akb_geometry.json"))
    res = dict(n=a.n, rays=a.n * a.n)
    for precision in ("fp64", "dd"):
        res[precision] = chain_rate(g, a.n, precision, a.reps)
    res["dd_over_fp64_time"] = res["dd"]["ms_median"] / res["fp64"]["ms_median"]
    print(json.dumps(res), flush=True)
    mode = {}
    with tempfile.TemporaryDirectory() as tmp:
        for flag in (False, True):
            times = []
            for rep in range(8):
                torch.cuda.synchronize()
                t = time.perf_counter()
                plot_result_ray_wave(best_params(), a.mode_size, directory=tmp, workdir=tmp, verbose=False,
                                     option_mpmath=flag)
                torch.cuda.synchronize()
                if rep:
                    times.append((time.perf_counter() - t) * 1e3)
            mode["option_mpmath" if flag else "fp64"] = dict(ms_median=float(np.median(times)), ms=times)
    res["ray_wave_mode"] = dict(size=a.mode_size, **mode)
    print(json.dumps(res["ray_wave_mode"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
