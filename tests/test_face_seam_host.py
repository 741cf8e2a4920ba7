"""scenes/face_textured.usda through a host integrator that textures from outside, without a GPU: the oracle's scalar
trace_path on its own traversal (OracleKernel) and untextured material functions, with tests/face_ref.py choosing the base
colour per hit (face_seam_host.FaceSeamHost over RefFaces). This is the truth image a device backend is compared with
(tests/test_gpu_face_seam_host.py); here the run is checked for what it must contain."""
import numpy as np
import pytest

import face_seam_host as fsh
import ora_world

load, truth_host = fsh.load_scene, fsh.truth_host


def test_the_scene_imports_as_it_is_meant_to(crt):
    desc = load(crt)
    kinds = {g["name"]: g for g in desc.geoms}
    assert kinds["Floor"]["kind"] == "mesh" and kinds["Floor"]["face_swapped"] is False
    assert kinds["Ceiling"]["kind"] == "mesh" and kinds["Ceiling"]["face_swapped"] is True  # mirrored, baked
    tiles = [kinds[n] for n in ("TileA", "TileB", "TileMoving")]
    assert all(t["kind"] == "instance" and t["face_swapped"] is False for t in tiles) and len({t["face_map"] for t in tiles}) == 1
    assert "l2w_end" in kinds["TileMoving"] and "l2w_end" not in kinds["TileA"]
    assert kinds["Ball"]["kind"] == "sphere" and kinds["Ball"]["material"]["_face_texture"] == 0 and "face_map" not in kinds["Ball"]
    assert 3 in desc.face_maps[kinds["Wall"]["face_map"]][1].tolist()  # the pentagon
    assert "_face_texture" not in kinds["Key"]["material"] and len(desc.face_textures) == 2


@pytest.mark.parametrize("case", ["moving", "static"])
def test_the_reference_integrator_meets_every_textured_case(crt, oracle, tmp_path, case):
    """Both cases of the scene: as it stands, and with the moving placement removed (nothing moves)."""
    desc = load(crt, static_dir=tmp_path if case == "static" else None)
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=8)
    assert (o.job.width, o.job.height) == (40, 24)
    host = truth_host(desc, o)
    img, st = host.render(o, 4, forward=1)
    assert host.errors == []  # every scatter / eval was about a hit the host knew
    for key, n in host.seen.items():
        assert n > 0, (key, host.seen)
    assert np.isfinite(img).all() and host.calls["intersect"] == st.closest_hit
    # the textures are in the picture: the same integrator on the authored colours gives another image
    plain, plain_st = o.render(4, threads=1, forward=1)
    assert (img.view(np.uint32) != plain.view(np.uint32)).any()
    assert st.camera_rays == plain_st.camera_rays == 40 * 24 * 4
