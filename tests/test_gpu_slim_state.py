"""The slim path state between two launches of the pipelined shade kernel (pathtrace.hip, k_shade_pipe<DRV, true>;
launch_plan.h, LaunchPlan::slim_state) against the full one (CRT_SLIM_STATE=0).

Where nothing in the material table emits, a pipelined launch hands the next one 48 bytes per path instead of 64: no
radiance (it is +0), no depth words (they follow from the bounce number), the hit word through the hit ring. What a path
computes does not change, so the frame's bits and all eight RayStats counters must be IDENTICAL with the knob at 0 and
unset, over every form the state is read from and handed over in: the three first-bounce input forms (compact, compact
with plane d under the root cull, full), the hand-over to the fused tail at its default bounce and right after the
first shade, no tail at all with the depth limit reached inside the slim form, one and three lanes, and an active-pixel
list (adaptive stopping). A table that holds an emitter must keep the full form."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

COUNTERS = ("camera_rays", "closest_hit", "shadow_rays", "vertices", "rr_tested", "rr_killed", "ended_escaped", "ended_depth")
EMITTER = os.path.join(ROOT, "tests", "golden", "cornellbox_emitter.usda")  # cornellbox, one sphere's material emits

CODE = (
    "import os, sys, numpy as np; sys.path.insert(0, %r); import torch\n"
    "from __graft_entry__ import load_package; crt = load_package()\n"
    "scene, depth, spp, batches, variance = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6])\n"
    "r, _ = crt.load_usda(crt.scene_path(scene), 96, 54, depth, variance=variance, min_spp=2 if variance else None)\n"
    "for b in range(batches): r.render_samples(b * spp, spp)\n"
    "p = r.pipeline(); lanes = r.lanes(); torch.cuda.synchronize(); st = r.stats()\n"
    "np.save(sys.argv[1], r.image())\n"
    "print(' '.join(str(getattr(st, k)) for k in %r), int(p['fused']), int(p['shade_pipe']), int(p['slim_state']), int(p['root_cull']), lanes)\n"
    % (ROOT, COUNTERS))


def run(tmp_path, tag, scene="cornellbox", depth=32, spp=8, batches=1, variance=0.0, **env):
    """One render in a fresh process (the knobs are read when the renderer is made): image, counters, pipeline."""
    path = str(tmp_path / ("img_%s.npy" % tag))
    base = dict(CRT_FUSED="0", CRT_STAGE_MIN_PATHS="1", CRT_LANE_MIN_PATHS="1")  # per-stage whatever the batch size; lanes split
    res = subprocess.run([sys.executable, "-c", CODE, path, scene, str(depth), str(spp), str(batches), str(variance)],
                         env=dict(os.environ, **{**base, **env}), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (tag, res.stderr[-2000:])
    line = [int(x) for x in res.stdout.strip().splitlines()[-1].split()]
    return np.load(path), tuple(line[:8]), dict(fused=line[8], shade_pipe=line[9], slim_state=line[10], root_cull=line[11], lanes=line[12])


def pair(tmp_path, slim_expected=1, **kw):
    """The same render with the form as the plan decides and with CRT_SLIM_STATE=0: same bits, same counters."""
    on, off = run(tmp_path, "on", **kw), run(tmp_path, "off", CRT_SLIM_STATE="0", **kw)
    assert on[2]["fused"] == 0 and on[2]["shade_pipe"] == 1 and on[2]["slim_state"] == slim_expected, on[2]
    assert off[2] == dict(on[2], slim_state=0), (on[2], off[2])
    assert on[1] == off[1], dict(zip(COUNTERS, zip(on[1], off[1])))
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    return on


@pytest.mark.parametrize("lanes", [1, 3])
def test_the_scene_s_own_depth_hands_over_to_the_tail(tmp_path, lanes):
    """Depth 32, the tail at its default bounce 12: eleven slim hand-overs, then the full form for k_path."""
    on = pair(tmp_path, depth=32, spp=9, CRT_LANES=str(lanes))
    assert on[2]["lanes"] == lanes
    assert on[1][4] > 0 and on[1][6] > 0  # roulette ran, paths escaped


def test_the_depth_limit_is_reached_inside_the_slim_form(tmp_path):
    """No tail, depth 3: the rebuilt `remaining` runs out at bounce 3, on hits and on misses, all with a previous vertex;
    depth 0 ends camera paths without one at the first shade."""
    on = pair(tmp_path, depth=3, spp=16, CRT_TAIL_FROM="0", CRT_LANES="1")
    assert on[1][7] > 0 and on[1][6] > 0  # paths ran out of depth, paths escaped
    on = pair(tmp_path, depth=0, spp=8, CRT_TAIL_FROM="0", CRT_LANES="1")
    assert on[1][7] > 0


def test_the_hand_over_right_after_the_first_shade(tmp_path):
    """CRT_TAIL_FROM=2: bounce 0 writes the slim form, bounce 1 reads it and writes the full one for the tail; with
    CRT_TAIL_FROM=1 the only pipelined launch writes the full form at once."""
    pair(tmp_path, depth=32, spp=8, CRT_TAIL_FROM="2", CRT_LANES="1")
    pair(tmp_path, depth=32, spp=8, CRT_TAIL_FROM="1", CRT_LANES="1")


@pytest.mark.parametrize("env", [dict(CRT_ROOT_CULL="0"), dict(CRT_ROOT_CULL="1"), dict(CRT_CAM_COMPACT="0")],
                         ids=["compact", "compact_d", "full"])
def test_the_three_first_bounce_input_forms(tmp_path, env):
    on = pair(tmp_path, depth=8, spp=8, CRT_LANES="1", **env)
    if "CRT_ROOT_CULL" in env:
        assert on[2]["root_cull"] == int(env["CRT_ROOT_CULL"])


def test_the_plain_shade_kernel_takes_over_from_the_full_form(tmp_path):
    """CRT_NOCLASSIFY_FROM=3, no tail: bounces 0-2 are pipelined (slim, slim, full), k_shade runs the rest."""
    pair(tmp_path, depth=8, spp=8, CRT_NOCLASSIFY_FROM="3", CRT_TAIL_FROM="0", CRT_LANES="1")


def test_an_active_pixel_list(tmp_path):
    """Adaptive stopping: after the first batches the pixel word is a slot of the active list."""
    pair(tmp_path, depth=8, spp=4, batches=4, variance=0.05, CRT_LANES="1")


def test_a_table_with_an_emitter_keeps_the_full_form(tmp_path):
    """One material of the scene emits: the pipelined instance runs, the plan keeps the full state, and radiance is
    carried (the frame is brighter than the scene without the emitter)."""
    on = pair(tmp_path, slim_expected=0, scene=EMITTER, depth=8, spp=8, CRT_LANES="1")
    plain = run(tmp_path, "plain", depth=8, spp=8, CRT_LANES="1")
    assert plain[2]["slim_state"] == 1
    assert on[0].sum() > plain[0].sum()
