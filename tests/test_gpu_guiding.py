"""The path guiding field on the device: crt_guiding_sample_n / crt_guiding_pdf_n on every named case and
crt_material_scatter_guided_n against the truth of tests/test_guiding.py — the float32 numpy restatement of guiding/*.rs
(tests/guiding_ref.py) and, for the bounce, that restatement composed with the oracle's drivers (tests/guiding_cases.py) —
bit for bit: at the block edges and a partial last block, with the hand-made edge list (NaN and infinite rows included),
on the default and on a non-default stream, across an update, and beside the untouched shading seam. The CPU half
(tests/test_guiding.py) pins the same source compiled for the host."""
import numpy as np
import pytest

import guiding_cases as gc
import guiding_ref as gr
import seam_cases as sc

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
N = 20000
SIZES = (1, 255, 256, 257)  # the block edge; the full list (N + the edge list) ends in a partial block


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.host(tmp_path_factory.mktemp("guiding_host"))


@pytest.fixture(scope="module")
def G(crt):
    import torch
    assert torch.cuda.is_available()
    return crt.guiding


def build(G, name, upto=None):
    cfg, passes = gc.case(name)
    field = G.GuidingField(gc.BMIN, gc.BMAX, G.GuidingConfig(**cfg))
    for samples, it in passes[:upto]:
        field.update(samples, it)
    return field


def device_answers(G, field, fn, q, stream=None):
    import torch
    d_q = G.to_device(q)
    torch.cuda.synchronize()
    if stream is None:
        out = getattr(field, fn)(d_q)
    else:
        with torch.cuda.stream(stream):
            out = getattr(field, fn)(d_q, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(gr.RESULT)


@pytest.mark.parametrize("name", gc.CASES)
def test_sample_and_pdf_bits_on_the_device(G, H, name):
    import torch
    field, ref = build(G, name), gc.build_ref(name, H)
    q = gc.queries(ref, N, 100 + gc.CASES.index(name))
    assert len(q) % 256 != 0 and len(q) > N
    side = torch.cuda.Stream()
    for fn in ("sample", "pdf"):
        want = getattr(ref, fn)(q)
        for stream in (None, side):
            got = device_answers(G, field, fn, q, stream)
            bad = gr.mismatches(got, want)
            assert len(bad) == 0, (name, fn, stream is not None, len(bad), q[bad[:2]], got[bad[:2]], want[bad[:2]])
        for n in SIZES:  # the last n rows: the hand-made list's NaN and infinite rows are among them
            got = device_answers(G, field, fn, q[-n:])
            assert len(gr.mismatches(got, want[-n:])) == 0, (name, fn, n)
    assert field.sample(G.to_device(q[:0])).numel() == 0  # n == 0


def test_update_then_query(G, H):
    """The device copy follows the field: answers after update 1 are the first state's, after update 2 the second's — and
    the identical sequence repeated in the same process gives identical bits."""
    runs = []
    for _ in range(2):
        cfg, passes = gc.case("octant")
        field, ref = G.GuidingField(gc.BMIN, gc.BMAX, G.GuidingConfig(**cfg)), gr.Field(gc.BMIN, gc.BMAX, cfg, H)
        q = gc.queries(ref, 4096, 9)
        answers = []
        for samples, it in passes[:2]:
            field.update(samples, it)
            ref.update(samples, it)
            for fn in ("sample", "pdf"):
                got, want = device_answers(G, field, fn, q), getattr(ref, fn)(q)
                assert len(gr.mismatches(got, want)) == 0, (it, fn)
                answers.append(got)
        assert len(gr.mismatches(answers[0], answers[2])) > 1000  # the second state answers differently
        runs.append(answers)
        field.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(u32), b.view(u32))


@pytest.mark.parametrize("fname", ("octant", "untrained"))
@pytest.mark.parametrize("cls", ("base", "transmission", "everything", "emissive"))
def test_guided_bounce_bits_on_the_device(crt, G, H, fname, cls):
    field, ref = build(G, fname), gc.build_ref(fname, H)
    rng = np.random.default_rng(3000 + sc.CLASSES.index(cls))
    mats = sc.materials(cls, 257, rng)
    q = sc.shade_queries(N, len(mats), rng)
    want, exits = gc.guided_truth(ref, mats, q)
    table = crt.shading.DeviceMaterials([crt.CrtMaterial.from_buffer_copy(m.tobytes()) for m in mats])
    d_q = crt.shading.to_device(q)
    got = table.scatter_guided(field, d_q).cpu().numpy().view(sc.SCATTER_SAMPLE)
    bad = sc.mismatches(got, want)
    assert len(bad) == 0, (fname, cls, len(bad), q[bad[:2]], got[bad[:2]], want[bad[:2]], exits[bad[:2]])
    if fname == "untrained":  # crt_material_scatter_n given the derived K_BSDF domain; flag bits 2 and 3 are 0 here too
        qb = q.copy()
        qb["sampler_pattern"] = gc.domains(q)[0]
        plain = table.scatter_importance(crt.shading.to_device(qb)).cpu().numpy().view(sc.SCATTER_SAMPLE)
        assert np.array_equal(got.view(u32), plain.view(u32)) and not (got["flags"] & 12).any()
    else:
        assert (got["flags"] & 4).all() and ((got["flags"] & 8) != 0).sum() == np.bincount(exits, minlength=5)[1]
        if cls != "emissive":
            assert ((got["flags"] & 8) != 0).mean() > 0.3
    for n in SIZES:  # block edges
        part = table.scatter_guided(field, crt.shading.to_device(q[:n])).cpu().numpy().view(sc.SCATTER_SAMPLE)
        assert np.array_equal(part.view(u32), got[:n].view(u32)), n


def test_the_existing_seam_is_untouched(crt):
    """crt_material_scatter_n / crt_material_eval_n on 4 096 `everything` queries still answer the oracle's bits."""
    rng = np.random.default_rng(4)
    mats = sc.materials("everything", 64, rng)
    q = sc.shade_queries(4096, len(mats), rng)
    table = crt.shading.DeviceMaterials([crt.CrtMaterial.from_buffer_copy(m.tobytes()) for m in mats])
    d_q = crt.shading.to_device(q)
    drv = sc.oracle_drivers()
    got_s = table.scatter_importance(d_q).cpu().numpy().view(sc.SCATTER_SAMPLE)
    got_e = table.eval(d_q).cpu().numpy().view(sc.BSDF_EVAL)
    assert len(sc.mismatches(got_s, drv.scatter(mats, q))) == 0 and len(sc.mismatches(got_e, drv.eval(mats, q))) == 0
    assert not (got_s["flags"] & 12).any()


def test_argument_checks_on_a_machine_with_a_device(crt, G):
    import torch
    L = crt.lib()
    g = G.GuidingField(gc.BMIN, gc.BMAX)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    assert L.crt_guiding_sample_n(None, p, 1, p, None) == -1 and L.crt_guiding_pdf_n(g.h, None, 1, p, None) == -1
    assert L.crt_material_scatter_guided_n(None, p, 1, p, 1, p, None) == -1
    assert L.crt_guiding_sample_n(g.h, None, 0, None, None) == 0
