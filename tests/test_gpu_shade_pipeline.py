"""The pipelined four-wave shade kernel (pathtrace.hip, shade_segment_pipe) against the plain one (CRT_SHADE_PIPE=0).

The pipelined instance reads a path's state once, through LDS staging blocks filled a step ahead, and finishes escaped
paths in a step of their own. Per-path arithmetic and film slots are shade_segment's; only the order in which a
workgroup takes its paths differs. So the frame's bits and all eight RayStats counters must be IDENTICAL with the knob on
and off — and the host must pick the instance by its LDS rule: unlit, simple materials, one material class, material
table within the arena; anything else keeps the plain kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

COUNTERS = ("camera_rays", "closest_hit", "shadow_rays", "vertices", "rr_tested", "rr_killed", "ended_escaped", "ended_depth")

CODE = (
    "import os, sys, numpy as np; sys.path.insert(0, %r); import torch\n"
    "from __graft_entry__ import load_package; crt = load_package()\n"
    "scene, w, h, depth, spp = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])\n"
    "r, _ = crt.load_usda(crt.scene_path(scene), w, h, depth)\n"
    "r.render_samples(0, spp); p = r.pipeline(); lanes = r.lanes(); r.render_samples(spp, 3); torch.cuda.synchronize(); st = r.stats()\n"
    "np.save(sys.argv[1], r.image())\n"
    "print(' '.join(str(getattr(st, k)) for k in %r), int(p['fused']), int(p['wide']), int(p['shade_pipe']), lanes)\n"
    % (ROOT, COUNTERS))


def run(tmp_path, tag, scene, w, h, depth, spp, **env):
    """One render in a fresh process (the knobs are read when the renderer is made): image, counters, pipeline, lanes."""
    path = str(tmp_path / ("img_%s.npy" % tag))
    # the per-stage pipeline with the four-wave kernels, whatever the batch size; lanes split down to one sample each
    base = dict(CRT_FUSED="0", CRT_WIDE="1", CRT_LANE_MIN_PATHS="1")
    res = subprocess.run([sys.executable, "-c", CODE, path, scene, str(w), str(h), str(depth), str(spp)],
                         env=dict(os.environ, **{**base, **env}), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (tag, res.stderr[-2000:])
    line = [int(x) for x in res.stdout.strip().splitlines()[-1].split()]
    return np.load(path), tuple(line[:8]), dict(fused=line[8], wide=line[9], shade_pipe=line[10], lanes=line[11])


def same(a, b):
    assert a[1] == b[1], dict(zip(COUNTERS, zip(a[1], b[1])))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# depth 2 and 3: paths escape with no depth left (ended_depth without a sky term) and hit at the depth limit; depth 32 is
# the scene's own, with Russian roulette and a fused tail
@pytest.mark.parametrize("depth", [2, 3, 8, 32])
@pytest.mark.parametrize("lanes", [1, 4])
def test_cornellbox_frame_and_counters_do_not_depend_on_the_shade_instance(tmp_path, depth, lanes):
    args = ("cornellbox", 160, 90, depth, 8)
    on = run(tmp_path, "on", *args, CRT_SHADE_PIPE="1", CRT_LANES=str(lanes))
    off = run(tmp_path, "off", *args, CRT_SHADE_PIPE="0", CRT_LANES=str(lanes))
    assert on[2] == dict(fused=0, wide=1, shade_pipe=1, lanes=lanes), on[2]
    assert off[2] == dict(fused=0, wide=1, shade_pipe=0, lanes=lanes), off[2]
    same(on, off)
    assert on[1][1] > 160 * 90 * 11 and on[1][6] > 0  # bounces happened, paths escaped
    if depth <= 3:
        assert on[1][7] > 0  # ... and paths ran out of depth


def test_an_odd_sized_batch_leaves_partial_steps(tmp_path):
    """A pixel count that is no multiple of the workgroup width, one sample: segments of a few paths, every step partial."""
    args = ("cornellbox", 37, 23, 6, 1)
    on = run(tmp_path, "on", *args, CRT_SHADE_PIPE="1", CRT_LANES="1")
    off = run(tmp_path, "off", *args, CRT_SHADE_PIPE="0", CRT_LANES="1")
    assert on[2]["shade_pipe"] == 1 and off[2]["shade_pipe"] == 0
    same(on, off)


def test_the_default_is_the_pipelined_instance_and_the_fused_pipeline_is_untouched(tmp_path):
    args = ("cornellbox", 96, 54, 8, 5)
    default = run(tmp_path, "default", *args)
    fused = run(tmp_path, "fused", *args, CRT_FUSED="1")
    assert default[2]["shade_pipe"] == 1
    assert fused[2]["fused"] == 1 and fused[2]["shade_pipe"] == 0
    same(default, fused)


@pytest.mark.parametrize("scene,depth", [("veach_mis", 8), ("cornellbox_guided", 6)])
def test_lit_scenes_of_several_material_classes_keep_the_plain_instance(tmp_path, scene, depth):
    """veach_mis and cornellbox_guided have lights (plane e would need a sixth staging plane) and emissive next to base
    materials (four class rings): by the LDS rule they run the plain kernel, knob or not, with the same results."""
    args = (scene, 96, 54, depth, 5)
    on = run(tmp_path, "on", *args, CRT_SHADE_PIPE="1", CRT_LANES="4")
    off = run(tmp_path, "off", *args, CRT_SHADE_PIPE="0", CRT_LANES="1")
    assert on[2]["shade_pipe"] == 0 and off[2]["shade_pipe"] == 0 and on[2]["fused"] == 0
    same(on, off)
    assert on[1][2] > 0  # shadow rays were traced


def test_a_partitioned_scene_keeps_the_plain_instance(tmp_path):
    """CRT_PARTITION=1 runs cornellbox with the class rings of a scene of several material classes: rings for four
    classes leave the pipelined instance no room for a material table, so the plain kernel runs."""
    args = ("cornellbox", 96, 54, 8, 5)
    part = run(tmp_path, "part", *args, CRT_SHADE_PIPE="1", CRT_PARTITION="1")
    plain = run(tmp_path, "plain", *args, CRT_SHADE_PIPE="1")
    assert part[2]["shade_pipe"] == 0 and plain[2]["shade_pipe"] == 1
    same(part, plain)
