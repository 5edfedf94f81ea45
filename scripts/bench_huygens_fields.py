"""Several fields per pass of the Huygens kernel against as many single-field calls (DESIGN.md
section 7.7): akb_huygens_fields_f64 for nf fields, and nf back-to-back calls of the unchanged
akb_huygens_f64, in one process, alternating, on the same seeded inputs, at two shapes:

  image:  n = 4225,  m = 1e7   the image stage of BASELINE config C2 (84.5 ms per single call, r03a)
  mirror: n = 65536, m = 1e6   mirror-stage-like: many target blocks, few splits

Device events around each call, the median (and min) of --reps after a warm-up of every shape and
nf; the rows of the last fields call are compared with the single calls bit for bit. Prints one
JSON line and writes it to --out.

    python scripts/bench_huygens_fields.py [--reps 5] [--nf 1,2,4,8,16] [--out profiles/r08a_huygens_fields.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"image": (4225, 10_000_000), "mirror": (65536, 1_000_000)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--nf", default="1,2,4,8,16")
    p.add_argument("--shapes", default="image,mirror")
    p.add_argument("--scale", type=float, default=1.0, help="shrink m (a rehearsal, not a measurement)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08a_huygens_fields.json"))
    a = p.parse_args()
    import numpy as np
    import torch
    from akbraytracing_amd import device as D
    from akbraytracing_amd.wavecalc import fields_per_pass, propagate, propagate_fields, splits_for
    dev = D.device()  # (fails without a GPU: there is no other way to take these numbers)
    nfs = [int(v) for v in a.nf.split(",")]
    k = 2 * np.pi / 13.5e-9
    res = {"metric": "Huygens-Fresnel fields per pass against single-field calls", "unit": "ms", "dtype": "f64",
           "device": torch.cuda.get_device_name(dev), "fields_per_pass": fields_per_pass(), "reps": a.reps,
           "shapes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for name in a.shapes.split(","):
        n, m = SHAPES[name]
        m = max(1, int(m * a.scale))
        gen = torch.Generator(device=dev).manual_seed(8)

        def box(count, z):  # a 1 mm box at (0, 0, z)
            pts = (torch.rand((3, count), dtype=torch.float64, device=dev, generator=gen) - 0.5) * 1e-3
            pts[2] += z
            return [pts[r].contiguous() for r in range(3)]

        t, s = box(n, 0.05), box(m, 0.0)
        U = torch.view_as_complex(torch.randn((max(nfs), m, 2), dtype=torch.float64, device=dev, generator=gen))
        rows = {}
        run_fields = lambda nf: propagate_fields(*t, *s, U[:nf], k)  # noqa: E731
        run_single = lambda nf: [propagate(*t, *s, U[f], k) for f in range(nf)]  # noqa: E731
        for nf in nfs:  # warm-up: every shape and nf of the timed window
            run_fields(nf), run_single(nf)
        torch.cuda.synchronize()
        times = {nf: ([], []) for nf in nfs}
        same = {}
        for _ in range(a.reps):
            for nf in nfs:  # alternate the two within a round
                ms_f, got = timed(lambda: run_fields(nf))
                ms_s, want = timed(lambda: run_single(nf))
                times[nf][0].append(ms_f)
                times[nf][1].append(ms_s)
                same[nf] = bool(torch.equal(torch.view_as_real(got).view(torch.int64),
                                            torch.view_as_real(torch.stack(want)).view(torch.int64)))
                del got, want
        for nf in nfs:
            f, one = times[nf]
            mf, ms = statistics.median(f), statistics.median(one)
            rows[str(nf)] = {"fields_ms": mf, "fields_min_ms": min(f), "singles_ms": ms, "singles_min_ms": min(one),
                             "fields_ms_per_field": mf / nf, "singles_ms_per_field": ms / nf, "speedup": ms / mf,
                             "rows_equal_bitwise": same[nf]}
        res["shapes"][name] = {"targets": n, "sources": m, "splits": splits_for(n, m), "nf": rows}
        del t, s, U
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
