"""What a batch launches, counted: crt_renderer_profile / crt_renderer_profile_read time every launch of a batch by class
(extend, shade, shadow, other) and count them. The counts follow from the launch plan (launch_plan.h, plan_launches) and
render_lane's loop: per stage with depth limit d and the tail from bounce t, extend = shade = min(d + 1, t); shadow
equals that on a lit scene under a strategy that samples the lights, else 0; other = generate + the tail launch when
t <= d + the film fold. Fused: one launch of class extend (the path-loop kernel), one other (the fold). The stats build
runs per stage without a tail. Whatever the pipeline, the image and the eight ray counters are the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = (
    "import os, sys, json, numpy as np; sys.path.insert(0, %r); import torch\n"
    "from __graft_entry__ import load_package; crt = load_package()\n"
    "depth, stats = int(sys.argv[2]), sys.argv[3] == '1'\n"
    "r, desc = crt.load_usda(crt.scene_path('cornellbox'), 48, 27, depth)\n"
    "r.set_lanes(1); r.profile(True)\n"
    "r.render_samples_stats(0, 2) if stats else r.render_samples(0, 2)\n"
    "torch.cuda.synchronize(); prof = r.profile_read(); st = r.stats(); p = r.pipeline()\n"
    "np.save(sys.argv[1], r.image())\n"
    "print(json.dumps(dict(launches={k: v['launches'] for k, v in prof.items()}, fused=p['fused'], lights=r.n_lights,\n"
    "                      strategy=r.settings.strategy, counters=[int(getattr(st, f)) for f, _ in st._fields_])))\n" % ROOT)


def expected(depth, tail_from, lit_sampled, fused=False, stats=False):
    if fused:
        return dict(extend=1, shade=0, shadow=0, other=1)
    tail = tail_from if (tail_from > 0 and not stats) else None
    bounces = depth + 1 if tail is None else min(depth + 1, tail)
    return dict(extend=bounces, shade=bounces, shadow=bounces if lit_sampled else 0,
                other=1 + (1 if tail is not None and tail <= depth else 0) + 1)


LIT_SAMPLED = False  # cornellbox.usda has no light (test_usd_scene.py): lit by the sky alone, so no shadow stage runs

CASES = [  # tag, environment, depth, stats build, fused, tail_from
    ("fused", dict(CRT_FUSED="1"), 6, False, True, 12),
    ("stage_tail3", dict(CRT_STAGE_MIN_PATHS="1", CRT_TAIL_FROM="3"), 6, False, False, 3),
    ("stage_notail", dict(CRT_STAGE_MIN_PATHS="1", CRT_TAIL_FROM="0"), 6, False, False, 0),
    ("stage_depth2", dict(CRT_STAGE_MIN_PATHS="1"), 2, False, False, 12),  # the tail is never reached
    ("fused_depth2", dict(CRT_FUSED="1"), 2, False, True, 12),             # ... what its image is compared with
    ("stats", dict(), 6, True, False, 12),
]


def test_launch_counts_follow_the_plan_and_the_pipelines_agree(tmp_path):
    import json
    outs = {}
    for tag, env, depth, stats, fused, tail_from in CASES:
        path = str(tmp_path / ("img_%s.npy" % tag))
        res = subprocess.run([sys.executable, "-c", CODE, path, str(depth), "1" if stats else "0"], env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (tag, res.stderr[-2000:])
        got = json.loads(res.stdout.strip().splitlines()[-1])
        print(tag, got["launches"], "fused", got["fused"], "lights", got["lights"], got["strategy"])
        assert got["fused"] == fused, (tag, got)
        assert got["lights"] == 0, (tag, got)
        assert got["launches"] == expected(depth, tail_from, LIT_SAMPLED, fused, stats), (tag, got)
        outs[tag] = (np.load(path), got["counters"])
    # one depth limit, however it is launched: the same image bits and the same eight counters
    assert outs["fused"][1][1] > 48 * 27 * 2  # bounces happened
    for tag, ref in (("stage_tail3", "fused"), ("stage_notail", "fused"), ("stats", "fused"), ("stage_depth2", "fused_depth2")):
        assert outs[tag][1] == outs[ref][1], tag
        assert np.array_equal(outs[tag][0].view(np.uint32), outs[ref][0].view(np.uint32)), tag
