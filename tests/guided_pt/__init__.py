"""The guiding-aware forward integrator (tests/guided_pt/guided_pt.c) behind ctypes — test infrastructure only.

Built at test time against oracle/_build/liboracle.so, as volume_pt builds its library. A GuidedIntegrator wraps an
ora_world.OracleRenderer (scene, tables, camera, settings: the oracle's own job) and renders it with a guiding field
bound through the function table: by default the host-compiled device source (guiding_ref.Host over the image
crt_guiding_image hands out: host_table), or Python callbacks into guiding_ref.Field composed with the oracle's scatter /
eval drivers (ref_table: guiding_cases.guided_truth, the composition test_guided_bounce_bits pins)."""
import ctypes as C
import os
import subprocess

import numpy as np

import ora

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fexcess-precision=standard", "-Wall", "-Wextra",
          "-Wno-unused-parameter", "-pthread", "-shared"]  # oracle/Makefile's

_vp = C.c_void_p
SCATTER_N = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp)
PDF_N = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t, _vp)
EXITS = ("untrained", "guide", "guide_fallback", "bsdf_delta", "bsdf_continuous")  # guiding_cases.EXITS


class GuideFns(C.Structure):
    _fields_ = [("image", _vp), ("scatter_n", _vp), ("pdf_n", _vp), ("alpha", C.c_float)]


class Coverage(C.Structure):
    _fields_ = [("exits", C.c_uint64 * 5)] + [(n, C.c_uint64) for n in ("nee_mixture", "nee_trained_no_eval", "primary_unguided",
                                                                         "post_medium_unguided")]

    def as_dict(self):
        d = {"exit_" + n: int(self.exits[k]) for k, n in enumerate(EXITS)}
        d.update({n: int(getattr(self, n)) for n, _t in self._fields_[1:]})
        return d


COVERAGE = tuple("exit_" + n for n in EXITS) + ("nee_mixture", "nee_trained_no_eval", "primary_unguided", "post_medium_unguided")


class Job(C.Structure):
    _fields_ = [("job", ora.RenderJob), ("guide", C.POINTER(GuideFns)), ("light_hooks", C.POINTER(ora.SeamHooks))]


_LIBS = {}


def lib(out_dir, plain_nee_pdf=False):
    """One build per directory and variant (a module- or session-scoped tmp dir in the tests). plain_nee_pdf: the WRONG
    variant (-DGPT_PLAIN_NEE_PDF), for the one test that shows the unbiasedness bound can fail."""
    key = (str(out_dir), bool(plain_nee_pdf))
    if key in _LIBS:
        return _LIBS[key]
    ora.lib()  # builds and loads liboracle.so
    odir = os.path.dirname(ora.LIB_PATH)
    out = os.path.join(key[0], "libguided_pt%s.so" % ("_plain_nee" if plain_nee_pdf else ""))
    cmd = ["gcc"] + CFLAGS + (["-DGPT_PLAIN_NEE_PDF"] if plain_nee_pdf else []) + [
        os.path.join(HERE, "guided_pt.c"), "-o", out, "-L" + odir, "-Wl,-rpath," + odir, "-loracle", "-lm", "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(out)
    L.gpt_render.restype = None
    L.gpt_render.argtypes = [C.POINTER(Job), _vp, _vp, C.POINTER(ora.RayStats), C.POINTER(Coverage), C.c_int]
    _LIBS[key] = L
    return L


def image_alpha(image_bytes):
    """guide_prob as the image's header states it (kernels/guiding.hip.h, GuideHeader::alpha: the ninth word)."""
    return float(np.ascontiguousarray(image_bytes, np.uint8)[:256].view(np.float32)[8])


def host_table(host, image_bytes):
    """The default function table: the device source compiled for the host (guiding_ref.Host), over a field's image (numpy
    uint8, GuidingField.image_bytes()). -> (GuideFns, what must stay alive with it)."""
    image = np.ascontiguousarray(image_bytes, dtype=np.uint8)
    fn = lambda name: C.cast(getattr(host.lib, name), _vp)
    t = GuideFns(image.ctypes.data, fn("host_guide_scatter_n"), fn("host_guide_pdf_n"), image_alpha(image))
    return t, (image, host)


def ref_table(field_ref):
    """The independent field: every call answered by the numpy restatement (guiding_ref.Field) — the bounce composed with
    the oracle's scatter / eval drivers as guiding_cases.guided_truth composes it. One query per call; render with one
    thread."""
    import guiding_cases as gc
    import guiding_ref as gr
    import seam_cases as sc

    def arr(ptr, n, dtype):
        return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=n)

    def scatter_n(_image, mats, n_mats, q, n, out):
        m, qs = arr(mats, n_mats, sc.MATERIAL), arr(q, n, sc.SHADE_QUERY)
        arr(out, n, sc.SCATTER_SAMPLE)[:] = gc.guided_truth(field_ref, m, qs)[0]

    def pdf_n(_image, q, n, out):
        arr(out, n, gr.RESULT)[:] = field_ref.pdf(arr(q, n, gr.QUERY))

    cbs = (SCATTER_N(scatter_n), PDF_N(pdf_n))
    t = GuideFns(None, C.cast(cbs[0], _vp), C.cast(cbs[1], _vp), float(field_ref.flat().alpha))
    return t, (cbs, field_ref)


class GuidedIntegrator:
    """guided_pt.c on the job of an ora_world.OracleRenderer. table: (GuideFns, keep-alive) from host_table / ref_table, or
    None for no field; light_hooks: an ora.SeamHooks whose three light members are used, or None."""

    def __init__(self, out_dir, oracle_renderer, table=None, light_hooks=None, plain_nee_pdf=False):
        self.L = lib(out_dir, plain_nee_pdf)
        self.o = oracle_renderer
        self.table = table
        self.light_hooks = light_hooks

    def _job(self, spp, variance=0.0, min_spp=None, frame=None):
        j = Job()
        C.memmove(C.byref(j.job), C.byref(self.o.job), C.sizeof(ora.RenderJob))
        j.job.spp = spp
        j.job.variance_threshold = float(variance)
        if min_spp is not None:
            j.job.min_spp = min_spp
        if frame is not None:
            j.job.frame = frame
        j.job.forward = 1
        j.guide = C.pointer(self.table[0]) if self.table is not None else None
        j.light_hooks = C.pointer(self.light_hooks) if self.light_hooks is not None else None
        return j

    def render(self, spp, threads=None, variance=0.0, min_spp=None, frame=None):
        """-> (image [h, w, 3], per-pixel sample counts [h, w], RayStats, coverage dict)."""
        j = self._job(spp, variance, min_spp, frame)
        h, w = j.job.height, j.job.width
        img = np.zeros((h, w, 3), np.float32)
        counts = np.zeros((h, w), np.uint32)
        st, cov = ora.RayStats(), Coverage()
        self.L.gpt_render(C.byref(j), img.ctypes.data, counts.ctypes.data, C.byref(st), C.byref(cov), threads or min(os.cpu_count() or 1, 16))
        return img, counts, st, cov.as_dict()
