"""What tests/test_guided_render.py and tests/test_gpu_guided_render.py share: a case's scene, field and restatement
(tests/guided_pt), built from tests/guided_render_cases.py. Test infrastructure only; nothing here needs a device."""
import numpy as np

import guided_pt as gp
import guiding_ref as gr
import ora
import ora_world

u32 = np.uint32


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def stats_tuple(st):
    return tuple(int(getattr(st, f)) for f, _t in ora.RayStats._fields_)


class Built:
    """A case's description, its oracle job, the scene's bounds and the training passes of its field."""

    def __init__(self, crt, case):
        self.case = case
        self.desc = case.desc(crt)
        self.o = ora_world.OracleRenderer(self.desc, crt.usda, max_depth=case.depth)
        self.bounds = self.o.scene.bounds()
        self.passes = case.passes(self.desc, self.bounds)

    def lib_field(self, crt, upto=None):
        """The field behind the ABI (host code, no device) after `upto` passes (all by default)."""
        g = crt.guiding.GuidingField(self.bounds[:3], self.bounds[3:], crt.guiding.GuidingConfig(**self.case.cfg))
        for samples, it in self.passes[:upto]:
            g.update(samples, it)
        return g

    def ref_field(self, host):
        """The numpy restatement's field from the same passes."""
        f = gr.Field(self.bounds[:3], self.bounds[3:], self.case.cfg, host)
        for samples, it in self.passes:
            f.update(samples, it)
        return f


def restatement(crt, work, built, table="host", image=None, light_hooks=None, plain_nee_pdf=False, spp=None, threads=None, frame=None):
    """guided_pt's render of a case -> (image, counts, stats tuple, coverage). table: "host" (the device source compiled
    for the host over the library's image — `image` overrides it), a (GuideFns, keep-alive) pair, or None (no field)."""
    case = built.case
    t = table
    if table == "host":
        if image is None:
            g = built.lib_field(crt)
            image = g.image_bytes()
            g.close()
        t = gp.host_table(gr.host(work), image)
    gi = gp.GuidedIntegrator(work, built.o, t, light_hooks=light_hooks, plain_nee_pdf=plain_nee_pdf)
    if light_hooks is not None or (t is not None and t[0].image is None):
        threads = 1  # Python callbacks
    img, counts, st, cov = gi.render(spp or case.spp, threads=threads, variance=case.variance, min_spp=case.min_spp, frame=frame)
    return img, counts, stats_tuple(st), cov
