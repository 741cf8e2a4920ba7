#!/usr/bin/env python3
"""Volume renders, first measurements: tests/golden/fog.usda and smoke.usda through crt_render_samples with their
aggregates bound (crt_renderer_set_volumes), 1920 x 1080, the scenes' own depth and strategy, adaptive stopping off.
    python profiles/volume_render_bench.py [--spp 32] [--reps 5] [--width 1920 --height 1080] [--out file.json]
Per scene: one warm-up batch, then `reps` batches of `spp` samples timed with device events around each call — Mray/s =
(closest-hit + shadow rays of the batch) / its time, median with the fastest and slowest beside it — and one more batch
under crt_renderer_profile for the per-class kernel times (extend / shade / shadow / other; the two volume kernels count
as "other"). The same batches with nothing bound give the surface-only figure of the same scene beside it. Needs the GPU
and a built library. There is no baseline for these: no earlier build renders volumes."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(crt, torch, path, w, h, spp, reps, bind):
    desc = crt.usda.load(path, w, h, volumes=True)
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(w, h, s["max_depth"], s["frame"], s["strategy"], s["filter"], s["filter_radius"], 0.0, s["min_spp"])
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r._protos = protos
    if bind:
        r.set_volumes(crt.usda.build_volumes(desc, crt))
    rays = lambda st: st.closest_hit + st.shadow_rays
    r.render_samples(0, spp)  # warm-up: buffers, code objects
    torch.cuda.synchronize()
    done, ms, mray = spp, [], []
    for _ in range(reps):
        before = rays(r.stats())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.render_samples(done, spp)
        e1.record()
        e1.synchronize()
        done += spp
        ms.append(e0.elapsed_time(e1))
        mray.append((rays(r.stats()) - before) / ms[-1] / 1e3)
    r.profile(True)
    r.render_samples(done, spp)
    torch.cuda.synchronize()
    prof = r.profile_read()
    r.profile(False)
    st, pipe = r.stats(), r.pipeline()
    return {"volumes": bool(bind), "regions": len(desc.volumes) if bind else 0, "depth": s["max_depth"], "strategy": s["strategy"],
            "pipeline": pipe, "lanes": r.lanes(), "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
            "mray_per_s_median": float(np.median(mray)), "mray_per_s_min": float(min(mray)), "mray_per_s_max": float(max(mray)),
            "rays_per_path": rays(st) / max(st.camera_rays, 1), "vertices_per_path": st.vertices / max(st.camera_rays, 1),
            "profile_one_batch": prof, "image_mean": float(r.image().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    crt = ge.load_package()
    result = {"what": "volume renders, first measurements (no baseline)", "width": a.width, "height": a.height, "spp_per_batch": a.spp,
              "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name in ("fog", "smoke"):
        path = os.path.join(ROOT, "tests", "golden", name + ".usda")
        result[name] = {"bound": run(crt, torch, path, a.width, a.height, a.spp, a.reps, True),
                        "unbound": run(crt, torch, path, a.width, a.height, a.spp, a.reps, False)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
