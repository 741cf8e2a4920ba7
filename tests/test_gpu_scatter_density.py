"""tests/test_scatter_density.py on the device: crt.shading.DeviceMaterials / DeviceLights draw and report, the same
chi-square and moment run on the device's own outputs, and the outputs equal the oracle's bit for bit, which is what
carries the oracle's statistics over. Twelve (material, view) pairs of N = 65 536 draws, every lobe class and every
Lambert configuration once, the four views spread over them."""
import numpy as np
import pytest

import scatter_density as sd
import seam_cases as sc
import test_scatter_density as cpu

pytestmark = pytest.mark.gpu

PAIRS = [(name, sd.VIEWS[(k + k // 4) % 4]) for k, name in enumerate(cpu.NAMES)]


class DeviceDrivers:
    """crt.shading behind the interface of seam_cases.Drivers (records in, records out)."""

    def __init__(self, crt):
        self.crt = crt

    def _materials(self, mats):
        return self.crt.shading.DeviceMaterials([self.crt.CrtMaterial.from_buffer_copy(m.tobytes()) for m in mats])

    def _lights(self, table):
        return self.crt.shading.DeviceLights((self.crt.CrtLight * len(table)).from_buffer_copy(table.tobytes()))

    def scatter(self, mats, q):
        return self._materials(mats).scatter_importance(self.crt.shading.to_device(q)).cpu().numpy().view(sc.SCATTER_SAMPLE)

    def eval(self, mats, q):
        return self._materials(mats).eval(self.crt.shading.to_device(q)).cpu().numpy().view(sc.BSDF_EVAL)

    def light_sample(self, table, q):
        return self._lights(table).sample_li(self.crt.shading.to_device(q)).cpu().numpy().view(sc.LIGHT_SAMPLE)


@pytest.fixture(scope="module")
def device(crt):
    return DeviceDrivers(crt)


@pytest.fixture(scope="module")
def oracle():
    return sc.oracle_drivers()


@pytest.mark.parametrize("name,cos_v", PAIRS)
def test_device_draws_have_the_reported_density(device, oracle, name, cos_v):
    s, _mean, _se = cpu.check_density(device, name, cos_v)
    assert len(sc.mismatches(s, sd.draws(oracle, sd.named(name), cos_v))) == 0


def test_device_light_pdfs_integrate_to_the_solid_angle(device, oracle):
    import radiometry_ref as rr
    for light, points, rec in ((0, cpu.SPHERE_POINTS, cpu.SPHERE), (1, cpu.RECT_POINTS, cpu.RECT)):
        for point in points:
            if light == 0:
                omega = rr.sphere_cap_solid_angle(np.linalg.norm(np.array(rec["center"]) - np.array(point, np.float64)), rec["radius"])
            else:
                omega = rr.rect_solid_angle(point, rec["origin"], rec["edge_u"], rec["edge_v"]) if point[1] < rec["origin"][1] else 0.0
            s = cpu.check_area_light(device, light, point, omega)
            assert len(sc.mismatches(s, sd.light_draws(oracle, cpu.TABLE, light, point))) == 0


def test_device_distant_and_dome_lights_sample_their_constant_pdf(device, oracle):
    cpu.test_distant_and_dome_lights_sample_their_constant_pdf(device)
    for light in (2, 3):
        got = sd.light_draws(device, cpu.TABLE, light, (1.0, 2.0, 3.0))
        assert len(sc.mismatches(got, sd.light_draws(oracle, cpu.TABLE, light, (1.0, 2.0, 3.0)))) == 0
