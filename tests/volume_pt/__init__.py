"""The volume-aware forward integrator (tests/volume_pt/volume_pt.c) behind ctypes — test infrastructure only.

Built at test time against oracle/_build/liboracle.so, as volume_ref.Host builds its library. A VolumeIntegrator wraps an
ora_world.OracleRenderer (scene, tables, camera, settings: the oracle's own job) and renders it with a volume aggregate
bound through the function table: by default the host-compiled device source (volume_ref.Host over the image
crt_volumes_image hands out), or Python callbacks into volume_ref.VolumesRef (ref_table)."""
import ctypes as C
import os
import subprocess

import numpy as np

import ora
import volume_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O2", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fexcess-precision=standard", "-Wall", "-Wextra",
          "-Wno-unused-parameter", "-pthread", "-shared"]  # oracle/Makefile's

_vp = C.c_void_p
INTERVALS_N = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t, _vp)
TRANSMITTANCE_N = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t, _vp)
SAMPLE_N = C.CFUNCTYPE(None, _vp, _vp, _vp, C.c_size_t, _vp)
HG_PHASE_N = C.CFUNCTYPE(None, _vp, _vp, C.c_size_t, _vp)


class VolumeFns(C.Structure):
    _fields_ = [("image", _vp), ("intervals_n", _vp), ("transmittance_n", _vp), ("sample_n", _vp), ("hg_phase_n", _vp)]


class Coverage(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("phase_vertices", "phase_nee", "depth_walks", "medium_walks", "phase_prev_hits",
                                          "phase_prev_escapes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _t in self._fields_}


class Job(C.Structure):
    _fields_ = [("job", ora.RenderJob), ("volumes", C.POINTER(VolumeFns)), ("light_hooks", C.POINTER(ora.SeamHooks))]


_LIBS = {}


def lib(out_dir):
    """One build per directory (a module- or session-scoped tmp dir in the tests)."""
    key = str(out_dir)
    if key in _LIBS:
        return _LIBS[key]
    ora.lib()  # builds and loads liboracle.so
    odir = os.path.dirname(ora.LIB_PATH)
    out = os.path.join(key, "libvolume_pt.so")
    cmd = ["gcc"] + CFLAGS + [os.path.join(HERE, "volume_pt.c"), "-o", out, "-L" + odir, "-Wl,-rpath," + odir, "-loracle", "-lm", "-lpthread"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(out)
    L.vpt_render.restype = None
    L.vpt_render.argtypes = [C.POINTER(Job), _vp, _vp, C.POINTER(ora.RayStats), C.POINTER(Coverage), C.c_int]
    L.vpt_render_sample.restype = None
    L.vpt_render_sample.argtypes = [C.POINTER(Job), C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.POINTER(ora.RayStats), C.POINTER(Coverage)]
    _LIBS[key] = L
    return L


def host_table(host, image_bytes):
    """The default function table: the device source compiled for the host (volume_ref.Host), over an aggregate's image
    (numpy uint8, crt.volumes.Volumes.image_bytes()). -> (VolumeFns, what must stay alive with it)."""
    image = np.ascontiguousarray(image_bytes, dtype=np.uint8)
    fn = lambda name: C.cast(getattr(host.lib, name), _vp)
    t = VolumeFns(image.ctypes.data, fn("host_vol_intervals_n"), fn("host_vol_transmittance_n"), fn("host_vol_sample_n"),
                  fn("host_vol_hg_phase_n"))
    return t, (image, host)


def ref_table(ref, host, V):
    """The independent walks: every call of the integrator answered by the numpy restatement volume_ref.VolumesRef
    (V: the package's volumes module, for the record dtypes). One query per call; render with one thread."""
    def arr(ptr, n, dtype):
        return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=n)

    def intervals_n(_image, q, n, out):
        q, o = arr(q, n, V.QUERY), arr(out, 18 * n, np.float32).reshape(n, 18)
        on, majorant, a, b = ref.active_intervals(q)
        mask = (on.astype(np.uint32) << np.arange(on.shape[1], dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
        o[:] = 0
        o[:, 0] = mask.view(np.float32)
        o[:, 1] = majorant
        o[:, 2:2 + 2 * on.shape[1]:2] = np.where(on, a, 0)
        o[:, 3:3 + 2 * on.shape[1]:2] = np.where(on, b, 0)

    def transmittance_n(_image, q, n, out):
        arr(out, n, V.TRANSMITTANCE)[:] = ref.transmittance(arr(q, n, V.QUERY), V.TRANSMITTANCE)

    def sample_n(_image, q, phase_u, n, out):
        pu = arr(phase_u, 3 * n, np.float32).reshape(n, 3) if phase_u else None
        arr(out, n, V.EVENT)[:] = ref.sample(arr(q, n, V.QUERY), pu, V.EVENT)

    def hg_phase_n(c, g, n, out):
        arr(out, n, np.float32)[:] = vr.hg_phase(host, arr(c, n, np.float32), arr(g, n, np.float32))

    cbs = (INTERVALS_N(intervals_n), TRANSMITTANCE_N(transmittance_n), SAMPLE_N(sample_n), HG_PHASE_N(hg_phase_n))
    t = VolumeFns(None, *[C.cast(cb, _vp) for cb in cbs])
    return t, (cbs, ref, host)


class VolumeIntegrator:
    """volume_pt.c on the job of an ora_world.OracleRenderer. table: (VolumeFns, keep-alive) from host_table / ref_table,
    or None for no aggregate; light_hooks: an ora.SeamHooks whose three light members are used, or None."""

    def __init__(self, out_dir, oracle_renderer, table=None, light_hooks=None):
        self.L = lib(out_dir)
        self.o = oracle_renderer
        self.table = table
        self.light_hooks = light_hooks

    def _job(self, spp, variance=0.0, min_spp=None):
        j = Job()
        C.memmove(C.byref(j.job), C.byref(self.o.job), C.sizeof(ora.RenderJob))
        j.job.spp = spp
        j.job.variance_threshold = float(variance)
        if min_spp is not None:
            j.job.min_spp = min_spp
        j.job.forward = 1
        j.volumes = C.pointer(self.table[0]) if self.table is not None else None
        j.light_hooks = C.pointer(self.light_hooks) if self.light_hooks is not None else None
        return j

    def render(self, spp, threads=None, variance=0.0, min_spp=None):
        """-> (image [h, w, 3], per-pixel sample counts [h, w], RayStats, coverage dict)."""
        j = self._job(spp, variance, min_spp)
        h, w = j.job.height, j.job.width
        img = np.zeros((h, w, 3), np.float32)
        counts = np.zeros((h, w), np.uint32)
        st, cov = ora.RayStats(), Coverage()
        self.L.vpt_render(C.byref(j), img.ctypes.data, counts.ctypes.data, C.byref(st), C.byref(cov), threads or (os.cpu_count() or 1))
        return img, counts, st, cov.as_dict()

    def render_sample(self, i, j_, sample, stats=None, cov=None):
        """One camera sample of pixel (i, j): radiance before the filter weight (ora_render_sample's counterpart)."""
        j = self._job(1)
        rgb = np.zeros(3, np.float32)
        st = stats if stats is not None else ora.RayStats()
        cv = cov if cov is not None else Coverage()
        self.L.vpt_render_sample(C.byref(j), i, j_, sample, rgb.ctypes.data, C.byref(st), C.byref(cv))
        return rgb
