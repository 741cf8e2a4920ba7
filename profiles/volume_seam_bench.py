#!/usr/bin/env python3
"""A seam micro-figure (not a render): queries per second of crt_volumes_transmittance_n and crt_volumes_sample_n on
smoke.usda's aggregate (tests/golden/smoke.usda: noise plume, homogeneous ember, 4x4x4 grid) at 2^22 seeded segments.
    python profiles/volume_seam_bench.py [--log2n 22] [--reps 300] [--out file.json]
Each entry point is warmed up with two launches, then timed launch by launch with device events; the figure is
queries / median launch time, with the fastest and slowest launch beside it. Needs the GPU and a built library."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import volume_cases as vc
    crt = ge.load_package()
    V = crt.volumes
    vol = crt.usda.build_volumes(crt.usda.load(os.path.join(ROOT, "tests", "golden", "smoke.usda"), volumes=True), crt)
    n = 1 << a.log2n
    q = vc.segments(V, n, 2022, (0.3, 1.7, -0.2), 4.0)
    d_q, d_pu = V.to_device(q), torch.from_numpy(vc.phase_numbers(n, 2023)).cuda()
    result = {"what": "seam micro-figure", "aggregate": "tests/golden/smoke.usda (3 regions)", "queries": n, "reps": a.reps,
              "device": torch.cuda.get_device_name(0)}
    for name, call in (("transmittance", lambda: vol.transmittance(d_q)), ("sample", lambda: vol.sample(d_q, d_pu))):
        for _ in range(2):
            out = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        rec = out.cpu().numpy().view(V.TRANSMITTANCE if name == "transmittance" else V.EVENT)
        result[name] = {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                        "window_s": float(ms.sum() / 1e3), "mqueries_per_s": float(n / np.median(ms) / 1e3),
                        "step_limited": int((rec["status"] != 0).sum())}
        if name == "sample":
            result[name]["scatters"] = int((rec["kind"] == 1).sum())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
