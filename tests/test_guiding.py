"""The path guiding field without a GPU: the host field behind crt_guiding_new / _update (csrc/guiding.cpp) and the device
source of kernels/guiding.hip.h compiled for the host (tests/host_shade/guiding_host.cpp) against the float32 numpy
restatement of guiding/{mod,dtree,sdtree,field}.rs (tests/guiding_ref.py) bit for bit — the image after EVERY update of
every named case, 20 000 random and a hand-made list of sample and pdf queries per case — the guided bounce
(sample_bounce_direction, tracer.rs:777-826) against a truth composed from that restatement and the oracle's drivers, the
twelve unit tests of guiding/*.rs ported with their counts and tolerances, the mixture's unbiasedness, every refusal of
crt_guiding_new, the argument checks of the device-facing calls, the importer's three settings, and a stand-alone
sanitizer program.

The statistical unit tests use numpy's random stream (the reference's openqmc::pcg::Rng is not in its tree), so they
re-check the statistics, not bits. Each prints the figure it asserts on; with the seeds below every one sits further than
a third of its tolerance from the bound (measured when the seeds were chosen)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guiding_cases as gc
import guiding_ref as gr
import seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
N = 20000
NAMES = ["untrained", "one_leaf", "octant", "sharp_cone", "deep_spatial", "one_point", "zero_flux", "edges"]
SYMBOLS = ["crt_guiding_config_default", "crt_guiding_new", "crt_guiding_free", "crt_guiding_update", "crt_guiding_image",
           "crt_guiding_stats", "crt_guiding_sample_n", "crt_guiding_pdf_n", "crt_material_scatter_guided_n"]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.host(tmp_path_factory.mktemp("guiding_host"))


@pytest.fixture(scope="module")
def G(crt):
    return crt.guiding


def image_differences(field, ref):
    """Names of the image's parts that differ from the restatement's flattened trees (bits)."""
    hd, sn, dn = field.image()
    fl = ref.flat()
    bad = []
    if len(dn) != len(fl.sums) or len(sn) != len(fl.axis):
        return ["counts"]
    for name, mine, theirs in (("sums", dn["sums"].view(u32), fl.sums.view(u32)), ("children", dn["children"].astype(np.int64), fl.children),
                               ("axes", sn["axis"].astype(np.int64), fl.axis), ("splits", sn["split"].view(u32), fl.split.view(u32)),
                               ("a", sn["a"].astype(np.int64), fl.a), ("b", sn["b"].astype(np.int64), fl.b),
                               ("bounds", np.r_[hd["bmin"], hd["bmax"]].view(u32), np.r_[fl.bmin, fl.bmax].view(u32))):
        if not np.array_equal(mine, theirs):
            bad.append(name)
    st = ref.stats()
    if (hd["magic"], hd["bytes"], hd["n_snodes"], hd["n_dnodes"], hd["n_dtrees"], hd["s_depth"], hd["d_depth"]) != \
            (0x44475243, len(field.image_bytes()), st["s_nodes"], st["d_nodes"], st["d_trees"], st["s_depth"], st["d_depth"]):
        bad.append("header")
    if hd["off_snodes"] != 256 or hd["off_dnodes"] % 256 or hd["off_dnodes"] < 256 + 16 * st["s_nodes"] or hd["alpha"] != f32(ref.cfg["guide_prob"]):
        bad.append("layout")
    return bad


@pytest.fixture(scope="module")
def built(G, H):
    """name -> the field over the ABI, the restatement, the image bytes, and what differed after each update."""
    out = {}
    for name in NAMES:
        cfg, passes = gc.case(name)
        field, ref = G.GuidingField(gc.BMIN, gc.BMAX, G.GuidingConfig(**cfg)), gr.Field(gc.BMIN, gc.BMAX, cfg, H)
        log = [(0, image_differences(field, ref), field.stats(), ref.stats())]
        for samples, it in passes:
            field.update(samples, it)
            ref.update(samples, it)
            log.append((it, image_differences(field, ref), field.stats(), ref.stats()))
        out[name] = dict(field=field, ref=ref, image=field.image_bytes(), log=log, cfg=cfg)
    return out


def test_the_case_list_is_the_one_named():
    assert list(gc.CASES) == NAMES


# ---- records and symbols -----------------------------------------------------------------------------------------------
def test_record_sizes_match_the_header(G, tmp_path):
    names = {"CrtGuidingConfig": G.CONFIG, "CrtGuidingSample": G.SAMPLE, "CrtGuidingQuery": G.QUERY, "CrtGuidingResult": G.RESULT,
             "CrtGuidingStats": G.STATS}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "crt_guiding.h"\nint main(void){' +
                   "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) +
                   'printf("caps %u %u %d\\n", CRT_GUIDING_MAX_DTREE_DEPTH, CRT_GUIDING_MAX_SPATIAL_DEPTH, CRT_GUIDING_MIN_RHO == 1.0f / 1024.0f);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    out = dict(line.split() for line in lines[:5])
    for n, dt in names.items():
        assert int(out[n]) == dt.itemsize, n
    assert [int(out[n]) for n in list(names)[:4]] == [24, 32, 32, 32]
    assert lines[5] == "caps 32 32 1" and (G.MAX_DTREE_DEPTH, G.MAX_SPATIAL_DEPTH, G.MIN_RHO) == (32, 32, 1 / 1024)


def test_the_header_declares_the_nine_entry_points_and_all_are_exported(crt):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crt_guiding.h")).read(), flags=re.S)
    names = re.findall(r"\b(crt_[a-z0-9_]+)\s*\(", text)
    assert sorted(names) == sorted(SYMBOLS) == sorted(crt.ABI_SYMBOLS_GUIDING) and len(set(names)) == 9
    for n in SYMBOLS:
        assert hasattr(crt.lib(), n), n
        assert n not in crt.ABI_SYMBOLS  # crt.h's list is untouched
    assert crt.guiding is not None and hasattr(crt.shading.DeviceMaterials, "scatter_guided")


def test_field_over_a_scenes_bounds(crt, G):
    b = crt.SceneBuilder()
    b.attach_sphere((1, 2, 3), 2.0)
    field = G.GuidingField.for_scene(b.commit())  # host-side build: no HIP call
    hd = field.image()[0]
    pad = f32(4.0) * f32(1e-3)  # field.rs:66: the widest extent * 1e-3, at least 1e-3
    assert np.array_equal(hd["bmin"], np.array([-1, 0, 1], f32) - pad) and np.array_equal(hd["bmax"], np.array([3, 4, 5], f32) + pad)
    assert G.GuidingField(np.zeros(3, f32), np.full(3, 0.5, f32)).image()[0]["bmax"][0] == f32(0.5) + f32(1e-3)
    with pytest.raises(ValueError):
        G.GuidingField.for_scene(crt.SceneBuilder().commit())


def test_config_default(G):
    d = G.GuidingConfig.default()
    assert (d.train_iterations, d.guide_prob, d.spatial_c, d.dtree_rho, d.dtree_max_depth, d.spatial_max_depth) == (4, 0.5, 4000.0, float(f32(0.01)), 20, 24)


# ---- update: the image after EVERY update is the restatement's flattened trees -----------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_image_and_tallies_after_every_update(built, name):
    b = built[name]
    assert len(b["log"]) == len(gc.case(name)[1]) + 1
    for it, bad, got, want in b["log"]:
        assert bad == [], (name, it, bad)
        assert got == want, (name, it, got, want)
    st = b["field"].stats()
    assert st["recorded"] == sum(len(s) for s, _ in gc.case(name)[1])
    if name == "deep_spatial":
        assert st["s_depth"] >= 6, st
    if name == "one_point":  # both trees reach the configured depths
        assert (st["s_depth"], st["d_depth"]) == (b["cfg"]["spatial_max_depth"], b["cfg"]["dtree_max_depth"]) == (5, 8), st
    if name == "zero_flux":  # counted — the spatial tree split — and never splat
        assert st["s_leaves"] > 1 and st["d_nodes"] == st["d_trees"] and not b["ref"].flat().sums.any()
    if name == "untrained":
        assert (st["s_nodes"], st["d_nodes"], st["d_depth"]) == (1, 1, 1)


# ---- queries: host twin == restatement, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sample_and_pdf_bits(built, H, name):
    b = built[name]
    q = gc.queries(b["ref"], N, 100 + NAMES.index(name))
    assert len(q) >= N + 2000
    for fn in ("sample", "pdf"):
        got, want = getattr(H, fn)(b["image"], q), getattr(b["ref"], fn)(q)
        bad = gr.mismatches(got, want)
        assert len(bad) == 0, (name, fn, len(bad), q[bad[:2]], got[bad[:2]], want[bad[:2]])
    s, p = b["ref"].sample(q), b["ref"].pdf(q)
    trained = name not in ("untrained", "zero_flux")
    assert s["some"].all() == trained and s["trained"].all() == trained and (s["some"] == s["trained"]).all() and (p["trained"] == s["trained"]).all()
    if trained:
        assert (s["pdf"] > 0).all() and (p["pdf"][:N] > 0).mean() > 0.05 and not (p["pdf"] < 0).any()
    else:
        assert not s["pdf"].any() and not p["pdf"].any()


def test_the_small_functions(H):
    rng = np.random.default_rng(3)
    c = rng.uniform(-2, 50, (1000, 3)).astype(f32)
    assert np.array_equal(H.luminance(c).view(u32), gr.luminance(c).view(u32))  # guiding/mod.rs:18-20
    for seed in (0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1):  # pcg_f32, dtree.rs:19-27
        state, want = np.array([seed], np.uint64), []
        for _ in range(64):
            state, u = gr.pcg_f32(state)
            want.append(u[0])
        got = H.pcg(seed, 64)
        assert np.array_equal(got.view(u32), np.array(want, f32).view(u32)) and (got >= 0).all() and (got < 1).all()
    maps = gr.Maps(H)
    d = np.concatenate([gc.unit(rng, 2000) * rng.uniform(0.1, 9, (2000, 1)).astype(f32), gc.edge_queries()["dir"][:224:16]])
    p0, p1 = maps.dir_to_canonical(d)
    assert len(gr.mismatches(H.dir_to_canonical(d), np.stack([p0, p1], axis=1))) == 0
    p = np.concatenate([rng.uniform(size=(2000, 2)), [[0, 0], [1, 1], [0.5, np.nan], [np.nan, 2.0], [0.25, -3.0]]]).astype(f32)
    assert len(gr.mismatches(H.canonical_to_dir(p), maps.canonical_to_dir(p[:, 0], p[:, 1]))) == 0
    assert np.isnan(H.canonical_to_dir(p)[-3, 2]) and H.canonical_to_dir(p)[-1, 0] == 0  # (1 - z * z).max(0): NaN and negatives -> 0


# ---- upstream's twelve unit tests (dtree.rs:300-458, sdtree.rs:200-243, field.rs:119-141) ------------------------------
ONE_TREE = dict(spatial_c=1e30)  # a spatial tree that never splits: the D-tree tests
CENTRE = np.zeros(3, f32)


def one_tree(G, passes):
    field = G.GuidingField(gc.BMIN, gc.BMAX, G.GuidingConfig(**ONE_TREE))
    for k, d in enumerate(passes):
        field.update(gc.make_samples(np.zeros((len(d), 3), f32), d), k + 1)
    assert field.stats()["s_leaves"] == 1
    return field


@pytest.fixture(scope="module")
def trained_tree(G):  # dtree.rs:331-344
    rng = np.random.default_rng(0xC0FFEE)
    return one_tree(G, [gc.octant_pass(rng, 20000) for _ in range(4)])


def test_ref_canonical_round_trip(H):
    d = gc.uniform_sphere(np.random.default_rng(11), 1000)
    back = H.canonical_to_dir(H.dir_to_canonical(d))
    err = np.linalg.norm(back.astype(np.float64) - d, axis=1).max()
    print("round trip", err)
    assert err < 1e-3


def test_ref_canonical_map_is_equal_area(H):
    z = H.canonical_to_dir(np.random.default_rng(12).uniform(size=(200000, 2)).astype(f32))[:, 2].astype(np.float64)
    print("mean z", z.mean(), "mean z2", (z * z).mean())
    assert abs(z.mean()) < 0.01 and abs((z * z).mean() - 1.0 / 3.0) < 0.01


def test_ref_pdf_integrates_to_one(H, trained_tree):
    d = gc.uniform_sphere(np.random.default_rng(13), 200000)
    pdf = H.dtree_pdf(trained_tree.image_bytes(), CENTRE, H.dir_to_canonical(d)).astype(np.float64)
    integral = 4.0 * np.pi * pdf.mean()
    print("integral", integral)
    assert abs(integral - 1.0) < 0.02


def test_ref_sample_pdf_matches_pdf_lookup(H, trained_tree):
    img = trained_tree.image_bytes()
    p, pdf, some = H.dtree_sample(img, CENTRE, np.random.default_rng(14).uniform(size=(1000, 2)))
    lookup = H.dtree_pdf(img, CENTRE, p)
    assert some.all() and (np.abs(pdf - lookup) < 1e-3 * (1.0 + pdf)).all()


def test_ref_samples_follow_flux(G, H):
    rng = np.random.default_rng(15)
    d = gc.uniform_sphere(rng, 10000)
    d[:, 2] = np.maximum(np.abs(d[:, 2]), 0.1)
    field = one_tree(G, [d])
    p, _, some = H.dtree_sample(field.image_bytes(), CENTRE, rng.uniform(size=(1000, 2)))
    z = H.canonical_to_dir(p)[:, 2]
    print("lowest z", z.min())
    assert some.all() and (z > -1e-3).all()


def test_ref_sampled_histogram_matches_pdf_on_sharp_tree(G, H):
    rng = np.random.default_rng(16)
    img = one_tree(G, [gc.cone_pass(rng, 50000) for _ in range(8)]).image_bytes()
    octant = lambda d: (d[:, 0] >= 0) + 2 * (d[:, 1] >= 0) + 4 * (d[:, 2] >= 0)
    n = 400000
    p, _, some = H.dtree_sample(img, CENTRE, rng.uniform(size=(n, 2)))
    freq = np.bincount(octant(H.canonical_to_dir(p)), minlength=8) / n
    d = gc.uniform_sphere(rng, n)
    pdf = H.dtree_pdf(img, CENTRE, H.dir_to_canonical(d)).astype(np.float64)
    mass = 4.0 * np.pi * np.bincount(octant(d), weights=pdf, minlength=8) / n
    print("octants", freq, mass)
    assert some.all() and (np.abs(freq - mass) < 0.02).all()


def test_ref_refinement_grows_hot_regions(trained_tree):
    assert trained_tree.stats()["d_depth"] > 2


def test_ref_untrained_tree_declines_to_sample(G, H):
    img = G.GuidingField(gc.BMIN, gc.BMAX).image_bytes()
    _, _, some = H.dtree_sample(img, CENTRE, np.array([[0.3, 0.9]], f32))
    assert not some.any() and H.dtree_pdf(img, CENTRE, np.array([[0.3, 0.7]], f32))[0] == 0.0


def line_samples(n):  # sdtree.rs:203-207
    t = (np.arange(n) % 100).astype(f32) / f32(100.0)
    return gc.make_samples(np.stack([t, np.full(n, 0.5, f32), np.full(n, 0.5, f32)], axis=1), np.tile(np.array([[0, 0, 1]], f32), (n, 1)))


def unit_field(G, **cfg):
    return G.GuidingField(np.zeros(3, f32), np.ones(3, f32), G.GuidingConfig(**cfg))


def test_ref_splits_after_enough_samples(G):
    field = unit_field(G, spatial_c=100.0)
    assert field.stats()["s_leaves"] == 1
    field.update(line_samples(5000), 1)  # threshold = 100 * sqrt(2) ~ 141 << 5000
    assert field.stats()["s_leaves"] > 1


def test_ref_children_inherit_parent_distribution(G, H):
    field = unit_field(G, spatial_c=100.0)
    field.update(line_samples(2000), 1)
    assert field.stats()["s_leaves"] > 1
    q = np.zeros(2, gr.QUERY)
    q["pos"], q["seed_u"], q["seed_v"] = [[0.1, 0.5, 0.5], [0.9, 0.5, 0.5]], [0.37, 0.81], [0.62, 0.14]
    r = H.sample(field.image_bytes(), q)
    assert r["trained"].all() and r["some"].all() and (r["dir"][:, 2] > 0).all()


def test_ref_no_split_below_threshold(G):
    field = unit_field(G, spatial_c=4000.0)
    field.update(gc.make_samples(np.full((50, 3), 0.5, f32), np.tile(np.array([[0, 0, 1]], f32), (50, 1))), 1)
    assert field.stats()["s_leaves"] == 1


def test_ref_field_trains_and_samples(G, H):
    field = unit_field(G)
    q = np.zeros(1, gr.QUERY)
    q["pos"], q["seed_u"], q["seed_v"] = 0.5, 0.3, 0.7
    r = H.sample(field.image_bytes(), q)
    assert not r["trained"][0] and not r["some"][0]
    pos = np.repeat(((np.arange(1000) % 10).astype(f32) / f32(10.0))[:, None], 3, axis=1)
    field.update(gc.make_samples(pos, np.tile(np.array([[0, 0, 1]], f32), (1000, 1))), 1)
    r = H.sample(field.image_bytes(), q)
    assert r["trained"][0] and r["some"][0] and r["pdf"][0] > 0 and r["dir"][0, 2] > 0
    q["dir"] = r["dir"]
    assert H.pdf(field.image_bytes(), q)["pdf"][0] > 0


# ---- the guided bounce: host twin == composed truth, tolerance zero, flags included ------------------------------------
BOUNCE_FIELDS = ("octant", "untrained", "sharp_cone")
_exits = {}


@pytest.mark.parametrize("fname", BOUNCE_FIELDS)
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_guided_bounce_bits(built, H, fname, cls):
    b = built[fname]
    rng = np.random.default_rng(3000 + sc.CLASSES.index(cls))
    mats = sc.materials(cls, 257, rng)
    q = sc.shade_queries(N, len(mats), rng)
    want, exits = gc.guided_truth(b["ref"], mats, q)
    got = H.scatter(b["image"], mats, q, sc.SCATTER_SAMPLE)
    bad = sc.mismatches(got, want)
    assert len(bad) == 0, (fname, cls, len(bad), q[bad[:2]], got[bad[:2]], want[bad[:2]], exits[bad[:2]])
    _exits[(fname, cls)] = np.bincount(exits, minlength=5)
    if fname == "untrained":  # 100 % take the first exit, and the answer is scatter_importance on the K_BSDF domain
        assert _exits[(fname, cls)][0] == N and not (got["flags"] & 12).any()
        assert len(sc.mismatches(got, H.plain_scatter(mats, q, sc.SCATTER_SAMPLE))) == 0
    else:
        assert (got["flags"] & 4).all() and ((got["flags"] & 8) != 0).sum() == _exits[(fname, cls)][1]


@pytest.mark.parametrize("fname", ("octant", "sharp_cone"))
def test_guided_bounce_cases_take_every_exit(built, H, fname):
    """The coverage condition, with the truth alone: over the classes together each of the four exits of a trained field
    is taken by at least 1 % of the calls (the delta exit by thin_wall and everything: no extra class was needed)."""
    total = np.zeros(5, np.int64)
    for cls in sc.CLASSES:
        if (fname, cls) not in _exits:
            rng = np.random.default_rng(3000 + sc.CLASSES.index(cls))
            mats = sc.materials(cls, 257, rng)
            _exits[(fname, cls)] = np.bincount(gc.guided_truth(built[fname]["ref"], mats, sc.shade_queries(N, len(mats), rng))[1], minlength=5)
        total += _exits[(fname, cls)]
    share = total / total.sum()
    print(fname, dict(zip(gc.EXITS, share)))
    assert share[0] == 0 and (share[1:] >= 0.01).all(), share


def test_guided_bounce_fails_with_fma_contraction(built, tmp_path_factory):
    """The same twin built with FMA contraction allowed does NOT reproduce the truth: the comparison above can fail."""
    fast = gr.host(tmp_path_factory.mktemp("guiding_host_fma"), "fast")
    rng = np.random.default_rng(3000)
    mats = sc.materials("base", 257, rng)
    q = sc.shade_queries(N, len(mats), rng)
    want, _ = gc.guided_truth(built["octant"]["ref"], mats, q)
    assert len(sc.mismatches(fast.scatter(built["octant"]["image"], mats, q, sc.SCATTER_SAMPLE), want)) > N // 100


# ---- the mixture is unbiased ---------------------------------------------------------------------------------------------
def mixture_material(kind):
    m = np.zeros(1, sc.MATERIAL)
    m["base_weight"], m["base_color"], m["base_diffuse_roughness"] = 1.0, (0.8, 0.6, 0.4), 0.3
    m["specular_weight"], m["specular_color"], m["specular_roughness"], m["specular_ior"] = 1.0, 1.0, 0.5, 1.5
    m["transmission_color"], m["transmission_dispersion_abbe_number"], m["geometry_opacity"] = 1.0, 20.0, 1.0
    m["subsurface_color"], m["subsurface_radius"], m["subsurface_radius_scale"] = 0.8, 1.0, (1.0, 0.5, 0.25)
    m["fuzz_color"], m["fuzz_roughness"], m["coat_color"], m["coat_ior"] = 1.0, 0.5, 1.0, 1.6
    m["thin_film_thickness"], m["thin_film_ior"] = 0.5, 1.4
    if kind == "rough_transmission":
        m["transmission_weight"], m["specular_roughness"] = 0.8, 0.9  # rough enough for every pdf to stay above the floor
    return m


@pytest.mark.parametrize("kind", ["base", "rough_transmission"])
def test_mixture_is_unbiased(built, H, kind, normal=(1, 1, 1)):
    """One hit record, one material, on `octant`: the mean of value / pdf over 2^18 guided draws equals the mean over 2^18
    scatter_importance draws within 5 standard errors of the difference, computed from the two samples themselves."""
    n = 1 << 18
    rng = np.random.default_rng(77)
    mats = mixture_material(kind)
    nrm = np.array(normal, np.float64)
    nrm = (nrm / np.linalg.norm(nrm)).astype(f32)
    q = np.zeros(n, sc.SHADE_QUERY)
    q["normal"], q["p"], q["t"], q["front_face"] = nrm, (1.0, 2.0, -1.5), 3.0, 1
    q["ray_dir"] = (-nrm + np.array([0.3, 0.1, -0.2], f32)).astype(f32)
    q["sampler_pattern"] = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(u32)
    q["sampler_index"] = rng.integers(0, 4096, size=n, dtype=u32)
    g = H.scatter(built["octant"]["image"], mats, q, sc.SCATTER_SAMPLE)
    p = H.plain_scatter(mats, q, sc.SCATTER_SAMPLE)
    assert (g["flags"] & 4).all() and 0.3 < ((g["flags"] & 8) != 0).mean() < 0.7 and not (g["flags"] & 1).any()
    if kind == "rough_transmission":  # continuous directions behind the normal, from the guide too
        below = np.einsum("ij,j->i", g["dir"], nrm) < 0
        assert (below & (g["some"] == 1)).mean() > 0.05 and (below & ((g["flags"] & 8) != 0)).sum() > 100
    # No draw hit the 1e-4 floor: the mixture pdf and scatter_importance's own pdf stay above it everywhere, and the BSDF
    # pdf behind the mixture (eval of the drawn direction) wherever the draw carries a value at all. The guide also
    # proposes directions the material cannot scatter into (the field's seeded cells reach beyond the trained octant:
    # below an opaque surface, outside the refraction cone) — there eval answers value 0 with its floored pdf, and a
    # contribution of exactly 0 is not changed by what it is divided by.
    qe = q.copy()
    qe["wi"] = np.where((g["some"] == 1)[:, None], g["dir"], q["wi"])
    ev = sc.oracle_drivers().eval(mats, qe)
    assert (g["pdf"][g["some"] == 1] > 1e-4).all() and (p["pdf"][p["some"] == 1] > 1e-4).all()
    carries = (g["some"] == 1) & (ev["some"] == 1) & (g["value"] != 0).any(axis=1)
    assert carries.mean() > 0.5 and (ev["pdf"][carries] > 1e-4).all()
    est = lambda r: np.where((r["some"] == 1)[:, None], r["value"].astype(np.float64) / np.maximum(r["pdf"], 1e-30)[:, None].astype(np.float64), 0.0)
    eg, ep = est(g), est(p)
    diff = eg.mean(axis=0) - ep.mean(axis=0)
    se = np.sqrt(eg.var(axis=0, ddof=1) / n + ep.var(axis=0, ddof=1) / n)
    print(kind, "means", eg.mean(axis=0), ep.mean(axis=0), "difference in standard errors", diff / se)
    assert (ep.mean(axis=0) > 0.05).all() and (np.abs(diff) <= 5.0 * se).all(), (diff, se)


# ---- refusals and argument checks ----------------------------------------------------------------------------------------
def test_every_refusal_returns_null_with_its_reason(crt, G):
    L = crt.lib()
    lo, hi = gc.BMIN.copy(), gc.BMAX.copy()

    def refused(reason, lo=lo, hi=hi, **cfg):
        rec = G.GuidingConfig(**cfg).record()
        h = L.crt_guiding_new(crt._fp(np.asarray(lo, f32)), crt._fp(np.asarray(hi, f32)), C.c_void_p(rec.ctypes.data))
        assert not h, (reason, cfg)
        assert reason in L.crt_last_error().decode(), (reason, L.crt_last_error())

    refused("bounds are not finite", lo=[np.nan, -5, -5])
    refused("bounds are not finite", hi=[5, np.inf, 5])
    refused("bounds are inverted on axis 1", hi=[5, -6, 5])
    for a in (0.0, 1.0, -0.25, 1.5, np.nan, np.inf):
        refused("is outside (0, 1)", guide_prob=a)
    for c in (0.0, -1.0, np.nan, np.inf):
        refused("spatial_c", spatial_c=c)
    for r in (0.0, -0.01, np.nan, np.inf):
        refused("dtree_rho", dtree_rho=r)
    refused("is below 1/1024", dtree_rho=1.0 / 2048.0)
    for d in (0, 33, 2 ** 32 - 1):
        refused("dtree_max_depth %d is outside 1 .. 32" % d, dtree_max_depth=d)
    for d in (33, 2 ** 32 - 1):
        refused("spatial_max_depth %d is above 32" % d, spatial_max_depth=d)
    assert not L.crt_guiding_new(None, crt._fp(hi), None) and b"NULL" in L.crt_last_error()
    with pytest.raises(crt.CrtError, match="guide_prob"):
        G.GuidingField(lo, hi, G.GuidingConfig(guide_prob=1.0))
    # the limits themselves are accepted, and so are degenerate (flat) bounds
    G.GuidingField(lo, hi, G.GuidingConfig(dtree_rho=1.0 / 1024.0, dtree_max_depth=32, spatial_max_depth=32, guide_prob=0.999)).close()
    G.GuidingField(lo, lo, G.GuidingConfig(spatial_max_depth=0, dtree_max_depth=1)).close()
    for _ in range(200):  # handles come and go
        G.GuidingField(lo, hi).close()


def test_argument_checks_of_the_device_facing_calls_need_no_device(crt, G):
    import torch
    L = crt.lib()
    g = G.GuidingField(gc.BMIN, gc.BMAX)
    for fn in (L.crt_guiding_sample_n, L.crt_guiding_pdf_n):
        assert fn(g.h, None, 0, None, None) == 0        # n == 0
        assert fn(g.h, None, 5, None, None) == -1 and fn(g.h, 1, 5, None, None) == -1 and fn(g.h, None, 5, 1, None) == -1
        assert fn(None, 1, 5, 1, None) == -1 and fn(None, None, 0, None, None) == -1
    sg = L.crt_material_scatter_guided_n
    assert sg(g.h, None, 0, None, 0, None, None) == 0 and sg(g.h, 1, 3, None, 0, None, None) == 0
    assert sg(g.h, 1, 3, None, 5, 1, None) == -1 and sg(g.h, 1, 3, 1, 5, None, None) == -1 and sg(g.h, None, 3, 1, 5, 1, None) == -1
    assert sg(None, 1, 3, 1, 5, 1, None) == -1 and sg(None, None, 0, None, 0, None, None) == -1  # the unguided call exists
    assert L.crt_guiding_update(None, None, 0, 1) == -1 and L.crt_guiding_update(g.h, None, 4, 1) == -1 and L.crt_guiding_update(g.h, None, 0, 1) == 0
    assert L.crt_guiding_image(None, None, None) == -1 and L.crt_guiding_stats(None, None) == -1 and L.crt_guiding_stats(g.h, None) == -1
    L.crt_guiding_free(None)  # as free(NULL)
    L.crt_guiding_config_default(None)
    if not torch.cuda.is_available():  # valid arguments: the first thing that needs a device says so
        assert L.crt_guiding_sample_n(g.h, 1, 5, 1, None) == -3 and L.crt_guiding_pdf_n(g.h, 1, 5, 1, None) == -3
        assert sg(g.h, 1, 3, 1, 5, 1, None) == -3


# ---- importer --------------------------------------------------------------------------------------------------------------
LAYER = """#usda 1.0
(defaultPrim = "W")
def Xform "W" { def Sphere "s" { double radius = 0.5 } def Camera "c" {} }
def Scope "Render" {
    def RenderSettings "settings" {
        int2 resolution = (32, 32)
        bool crust:pathGuiding = true
        int crust:guidingTrainIterations = 0
        float crust:guidingProb = 0.97
    }
}
"""


def test_importer_reads_the_three_settings_only_when_asked(crt, tmp_path):
    keys = lambda d: (d.settings["guiding"], d.settings["guiding_train_iterations"], d.settings["guiding_prob"])
    guided = os.path.join(ROOT, "scenes", "cornellbox_guided.usda")
    assert keys(crt.usda.load(guided, path_guiding=True)) == (True, 8, 0.5)
    plain = crt.usda.load(guided)
    assert sorted(plain.settings) == ["filter", "filter_radius", "frame", "height", "max_depth", "min_spp", "spp", "strategy", "variance", "width"]
    with_flag = crt.usda.load(guided, path_guiding=True)
    assert {k: v for k, v in with_flag.settings.items() if not k.startswith("guiding")} == plain.settings
    assert keys(crt.usda.load(os.path.join(ROOT, "scenes", "cornellbox.usda"), path_guiding=True)) == (False, 4, 0.5)
    layer = tmp_path / "inline.usda"
    layer.write_text(LAYER)
    d = crt.usda.load(str(layer), path_guiding=True)
    assert keys(d) == (True, 1, 0.9)
    assert "guiding" not in crt.usda.load(str(layer)).settings


# ---- sanitizers: a stand-alone program, on the CPU -------------------------------------------------------------------------
def test_field_updates_refusals_and_descents_are_clean_under_asan_and_ubsan(tmp_path):
    """profiles/host_shade/guiding_sanitize.cpp: guiding.cpp's new / update / refine / flatten and the host-compiled
    descents in a program of their own (its own main), built with -fsanitize=address,undefined; nothing of it is loaded
    into Python."""
    exe = tmp_path / "guiding_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "profiles", "host_shade"),
           "-I" + os.path.join(ROOT, "crust-render_amd", "csrc"), os.path.join(ROOT, "profiles", "host_shade", "guiding_sanitize.cpp"),
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "guiding_sanitize: 25 refusals, 5 fields, 105600 descents, 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
