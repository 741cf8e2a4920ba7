"""The derived material records change no bit (kernels/shade.hip.h, MatDerived; pathtrace.hip, k_derive_materials).

The shade kernels of simple-material scenes read the per-material constants of the vertex code from records derived once
per renderer; CRT_MAT_DERIVED=0 launches the instances that compute them at every vertex from the raw records, as every
build before did. Same IEEE operations on the same inputs, so the frame bits and all eight counters must be identical —
on the bench scene (cornellbox: the pipelined four-wave shade kernel per stage, k_path fused), on lit simple-material
scenes (veach_mis, cornellbox_guided, stress: k_shade and k_path with mat_eval and mat_scatter per vertex), and on
openpbr_showcase, the scene with every lobe and interior media, whose general instances keep the raw records either way.
The function-level statement of the same, without a GPU, is tests/test_shading_derived_host.py."""
import numpy as np
import pytest

import ora

pytestmark = pytest.mark.gpu

SCENES = [("cornellbox", 160, 90, 8), ("veach_mis", 160, 90, 8), ("openpbr_showcase", 96, 54, 12),
          ("cornellbox_guided", 96, 96, 8), ("stress", 96, 54, 6)]


def _render(crt, scene, w, h, depth):
    import torch
    r, _ = crt.load_usda(crt.scene_path(scene), w, h, depth)
    r.render_samples(0, 5)
    r.render_samples(5, 3)
    torch.cuda.synchronize()
    st = r.stats()
    return r.image(), [getattr(st, f) for f, _t in ora.RayStats._fields_], r.pipeline()


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("scene,w,h,depth", SCENES)
def test_derived_records_change_no_bit(crt, monkeypatch, scene, w, h, depth, fused):
    monkeypatch.setenv("CRT_FUSED", fused)
    monkeypatch.setenv("CRT_MAT_DERIVED", "0")
    raw_img, raw_st, raw_pipe = _render(crt, scene, w, h, depth)
    monkeypatch.delenv("CRT_MAT_DERIVED")
    img, st, pipe = _render(crt, scene, w, h, depth)
    assert len(st) == 8 and st == raw_st, (scene, fused, st, raw_st)
    assert st[1] > w * h * 8  # closest-hit rays beyond the camera rays: bounces happened
    assert np.array_equal(img.view(np.uint32), raw_img.view(np.uint32)), (scene, fused)
    assert pipe == raw_pipe and pipe["fused"] == (fused == "1")
    if scene == "cornellbox" and fused == "0":  # the bench's shade kernel is the one compared here
        assert pipe["shade_pipe"], pipe
