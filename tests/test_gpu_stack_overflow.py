"""The traversal stack's overflow path (traverse_pool.hip.h, CRT_ERR_STACK) on the GPU. A ray has one device stack for
every instance level and its leaf words; the shipped build holds 255 entries, which no test scene reaches. So this test
builds the library with a private part of ONE entry (-DCRT_POOL_SPILL=1, the LDS part unchanged) into a temporary
directory and runs it in a child process (CRT_AMD_LIB): on a scene whose oracle stack high water is far above that
capacity the batched queries complete and the scene's error word reports CRT_ERR_STACK, as do the _stats and single-ray
forms; on a scene that never leaves the LDS part of the stack the same build reports nothing and matches the oracle
bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as g
import fixtures as fx
import ora
crt = g.load_package()
import torch
assert crt.LIB_PATH == %(lib)r

def soup(api, n):
    rng = np.random.default_rng(5)
    c = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    v = (c[:, None, :] + rng.uniform(-6, 6, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    b = api.SceneBuilder()
    b.attach_triangles(v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))
    return b.commit()

def shallow(api):
    b = api.SceneBuilder()
    b.attach_triangles(np.array([(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)], np.float32),
                       np.array([(0, 1, 2), (0, 2, 3)], np.uint32))
    b.attach_sphere((0.0, 0.0, 2.0), 1.0)
    return b.commit()

def code(f):
    try:
        f()
        return 0
    except crt.CrtError as e:
        return e.code

out = {}
rays = fx.ray_batch(2048, 12.0)
o_deep = soup(ora, 8000)
st = ora.TravStats()
ora.lib().ora_set_trav_stats(C.byref(st))
o_deep.intersect_n(rays, 0.001, float("inf"))
ora.lib().ora_set_trav_stats(None)
out["oracle_high_water"] = int(st.stack_high_water)
deep = soup(crt, 8000)
out["lds_stack"] = deep.engine_select(-2)["lds_stack"]
d_rays = crt.rays_to_device(rays)
hits = crt.hits_to_host(deep.intersect_n(d_rays, 0.001, float("inf")))
occ = deep.occluded_n(d_rays, 0.001, float("inf")).cpu().numpy()
torch.cuda.synchronize()
out["batched_completed"] = int(hits.shape[0]) == 2048 and int(occ.shape[0]) == 2048
out["batched_error"] = code(lambda: deep.traversal_error())
out["error_cleared"] = code(lambda: deep.traversal_error())
out["stats_error"] = code(lambda: deep.intersect_n(d_rays, 0.001, float("inf"), stats=crt.CrtTravStats()))
out["stats_any_error"] = code(lambda: deep.occluded_n(d_rays, 0.001, float("inf"), stats=crt.CrtTravStats()))
single = []
for i in range(64):
    r = crt.Ray(rays[i, 0:3], rays[i, 3:6])
    single.append(code(lambda: deep.intersect(r, 0.001, float("inf"))))
out["single_errors"] = sorted(set(single))
code(lambda: deep.traversal_error())  # whatever the single-ray launches left

o_sh, p_sh = shallow(ora), shallow(crt)
rays = fx.ray_batch(2048, 6.0)
hf, ids, front = o_sh.intersect_n(rays, 0.001, float("inf"))
o_occ = o_sh.occluded_n(rays, 0.001, float("inf"))
d_rays = crt.rays_to_device(rays)
h = crt.hits_to_host(p_sh.intersect_n(d_rays, 0.001, float("inf")))
g_occ = p_sh.occluded_n(d_rays, 0.001, float("inf")).cpu().numpy()
torch.cuda.synchronize()
hit = ids[:, 0] != 0xFFFFFFFF
out["shallow_hits"] = int(hit.sum())
out["shallow_equal"] = bool(np.array_equal(h["geom_id"], ids[:, 0]) and np.array_equal(h["prim_id"], ids[:, 1])
                            and np.array_equal(h["t"][hit].view(np.uint32), hf[hit, 0].view(np.uint32))
                            and np.array_equal(h["normal"][hit].view(np.uint32), hf[hit, 1:4].view(np.uint32))
                            and np.array_equal(g_occ.astype(np.uint8), o_occ))
out["shallow_error"] = code(lambda: p_sh.traversal_error())
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def small_stack_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("spill1")
    lib = str(d / "libcrt_amd_spill1.so")
    jobs = str(min(16, os.cpu_count() or 1))
    res = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "crust-render_amd", "csrc"), "-j" + jobs,
                          "OUT=" + lib, "OBJDIR=" + str(d / "obj"), "EXTRA=-DCRT_POOL_SPILL=1"],
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and os.path.exists(lib), res.stderr[-3000:]
    return lib


def test_stack_overflow_is_reported_and_harmless(small_stack_lib):
    env = dict(os.environ, CRT_AMD_LIB=small_stack_lib)
    script = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "lib": small_stack_lib}
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-3000:])
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    capacity = out["lds_stack"] + 1
    assert out["oracle_high_water"] >= capacity + 5, out  # well above: the device stack also holds leaf words
    assert out["batched_completed"], out
    assert out["batched_error"] == -4 and out["error_cleared"] == 0, out  # CRT_ERR_STACK, then read and cleared
    assert out["stats_error"] == -4 and out["stats_any_error"] in (0, -4), out  # any hit may stop before the overflow
    assert -4 in out["single_errors"] and set(out["single_errors"]) <= {0, -4}, out
    assert out["shallow_hits"] > 500 and out["shallow_equal"] and out["shallow_error"] == 0, out
