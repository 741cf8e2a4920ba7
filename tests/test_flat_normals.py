"""The unit normal a flat triangle carries in the device image (dev_image.h, flat_tri_normal; scene.cpp,
flatten_image), checked on the host: crt_scene_image_check re-evaluates every stored normal, and the records themselves
(crt_scene_image_prims) are compared here with a float32 evaluation of prim.rs:76-95 that shares no code with the
library. No GPU."""
import numpy as np
import pytest

import packet_cases as pc

f32 = np.float32
SMOOTH_TAG = 0x7FA5A5A5  # dev_image.h, kSmoothNormalTag: a signalling NaN, which no division returns


def _mixed_mesh():
    """40 flat triangles (a 4 x 5 grid, bent out of its plane), one of them zero-area, and 24 smooth ones."""
    rng = np.random.default_rng(21)
    gx, gy = np.meshgrid(np.arange(6, dtype=f32), np.arange(5, dtype=f32))
    v = np.stack([gx.ravel(), gy.ravel(), rng.uniform(-0.5, 0.5, gx.size).astype(f32)], axis=1).astype(f32)
    idx = []
    for j in range(4):
        for i in range(5):
            a = j * 6 + i
            idx += [(a, a + 1, a + 7), (a, a + 7, a + 6)]
    idx[7] = (idx[7][0], idx[7][1], idx[7][1])  # a repeated vertex: zero area
    sv, si = pc.fx.uv_sphere((8.0, 2.0, 0.0), 1.0, 4, 3)
    sn = sv - np.array([8.0, 2.0, 0.0], f32)
    sn = (sn / np.maximum(np.linalg.norm(sn, axis=1, keepdims=True), 1e-20)).astype(f32)
    return (v, np.array(idx, np.uint32)), (sv, si, sn)


def _build(crt, instanced):
    (v, i), (sv, si, sn) = _mixed_mesh()
    b = crt.SceneBuilder()
    b.attach_triangles(v, i)
    b.attach_triangles(sv, si, normals=sn)
    scene = b.commit()
    if not instanced:
        return scene, [scene]
    top = crt.SceneBuilder()
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], f32) * f32(1.5)
    top.attach_instance(scene, crt.affine(rot, (3.0, -2.0, 1.0)))
    top.attach_triangles(v + f32(20.0), i)
    return top.commit(), [scene]


@pytest.mark.parametrize("instanced", [False, True])
def test_flat_triangles_store_their_geometric_normal_bitwise(crt, instanced):
    scene, _keep = _build(crt, instanced)
    chk = scene.image_check()  # verifies every stored normal against a fresh flat_tri_normal
    assert chk["instances"] == (1 if instanced else 0)
    prims = scene.image_prims()
    tri = prims[prims[:, 0] == 0]
    assert len(tri) == (40 + 24) + (40 if instanced else 0)
    smooth = tri[:, 14] == SMOOTH_TAG
    assert int(smooth.sum()) == 24 and len(np.unique(tri[smooth, 13])) == 24  # one slot each
    flat = tri[~smooth]
    want = pc.flat_normal_f32(flat[:, 4:13].view(f32))
    got = flat[:, 13:16].view(f32)
    ok = np.isfinite(want).all(axis=1)
    assert int((~ok).sum()) == (2 if instanced else 1)  # the zero-area triangle: 0 / 0, never emitted (Tri4::normal_ok)
    assert np.isnan(got[~ok]).all()
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    assert np.abs(np.linalg.norm(got[ok].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    # the tag is no value the arithmetic can return: every stored word of a flat record differs from it
    assert not (flat[:, 13:16] == SMOOTH_TAG).any()
    sel = scene.engine_select(-1)
    assert sel["cold"] & 1  # shading normals present: the kernels with the interpolating arm (kColdUV)


def test_an_image_without_shading_normals_selects_the_kernels_without_the_smooth_arm(crt):
    (v, i), _ = _mixed_mesh()
    b = crt.SceneBuilder()
    b.attach_triangles(v, i)
    scene = b.commit()
    scene.image_check()
    prims = scene.image_prims()
    assert len(prims) == 40 and not (prims[:, 14] == SMOOTH_TAG).any()
    sel = scene.engine_select(-1)
    assert sel["cold"] & 1 == 0 and sel["ext_cold"] & 1 == 0 and sel["path_cold"] & 1 == 0


@pytest.mark.parametrize("name", pc.NAMES)
def test_packet_case_scenes_pass_the_image_check(crt, name):
    """The scenes of tests/test_gpu_packet_step.py: image self-check, and what each is built to contain."""
    scene, _mats, _protos = pc.World(crt.usda).build_world(pc.desc(crt.usda, name), crt, crt.default_material)
    scene.image_check()
    _n, _l, packets, _i, counts = scene.tree()
    active, mask_and, mask_or = packets[:, 40], packets[:, 41], packets[:, 42]
    if name == "masks":
        for m in (pc.CAMERA, pc.SHADOW):  # mask_and does not decide: the per-lane masks are fetched
            assert int(((active != 0) & ((mask_and & m) == 0) & ((mask_or & m) != 0)).sum()) >= 1, m
        assert int(((mask_and & pc.INDIRECT) != 0).sum()) >= 1
    if name == "stack":
        four = [p for p in packets if bin(int(p[40])).count("1") == 4 and len({int(x) for x in p[36:40]}) == 4]
        z = [sorted(p[8:12].view(f32).tolist()) for p in four]  # v0.z of the four lanes
        assert [0.0, 1.0, 2.0, 3.0] in z, z  # the four parallel triangles share one packet
    if name == "normals":
        prims = scene.image_prims()
        tri = prims[prims[:, 0] == 0]
        assert int((tri[:, 14] == SMOOTH_TAG).sum()) == 100 and len(tri) > 300
        assert scene.engine_select(-1)["cold"] & 3 == 3  # shading normals, and a second instance level
