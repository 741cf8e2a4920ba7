/* TEST INFRASTRUCTURE ONLY: a volume-aware forward integrator, the truth the wavefront renderer's volume renders are
 * compared with bit for bit (tests/test_volume_render.py, tests/test_gpu_volume_render.py).
 *
 * The oracle (oracle/ora_pt.c) knows no volume region. This file restates camera_sample, render_pixel (adaptive rule
 * included) and trace_path (tracer.rs:515-636, :1086-1558) in the oracle's FORWARD form, extended by the volume-forward
 * form of DESIGN.md §2 (tracer.rs:1016-1076, :1138-1141, :1167-1254), on the oracle's exported functions: ora_intersect /
 * ora_occluded, ora_mat_*, ora_light_*, ora_camera_get_ray, ora_filter_sample, ora_qmc.h, the medium functions,
 * ora_light_weight and ora_bounce_weight. With no aggregate bound, or one no ray crosses, it is the oracle's forward
 * mode operation for operation (test_volume_render.py pins that on three scenes).
 *
 * The two walks and the phase sample are reached through a function table (VptVolumeFns): four batch functions with the
 * signatures of tests/host_shade/volume_host.cpp — the device source compiled for the host, itself pinned to the numpy
 * restatement tests/volume_ref.py — called with n = 1. The table may instead hold Python callbacks into
 * volume_ref.VolumesRef (one thread then).
 *
 * Built at test time by tests/volume_pt/__init__.py against oracle/_build/liboracle.so. */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/crt.h"
#include "../../oracle/ora_pt.h"

enum { K_CAMERA = 0, K_PATH = 1, K_TIME = 2 };                                                                  /* tracer.rs:20-22 */
enum { K_NEE = 0, K_NEE_SHADOW = 1, K_BSDF = 2, K_GUIDE = 3, K_PHASE = 4, K_RR = 5, K_MEDIUM = 6, K_VOLUME = 7 }; /* :23-30 */
#define RR_START_BOUNCE 3 /* tracer.rs:46 */
#define RR_MIN_PROB 0.05f /* tracer.rs:47 */

typedef struct VptVolumeFns {
  const void *image; /* handed back as the first argument: the aggregate's byte image, or any context */
  /* per query 18 floats: mask (u32 bits), majorant, 8 x (a, b) — Volumes::active_intervals */
  void (*intervals_n)(const void *image, const CrtVolumeQuery *q, size_t n, float *out);
  void (*transmittance_n)(const void *image, const CrtVolumeQuery *q, size_t n, CrtVolumeTransmittance *out);
  /* phase_u: 3 floats per query (lobe_u, hg_u, hg_v): dir / pdf of a scatter are PhaseMix::sample and max(pdf, 1e-6) */
  void (*sample_n)(const void *image, const CrtVolumeQuery *q, const float *phase_u, size_t n, CrtVolumeEvent *out);
  void (*hg_phase_n)(const float *cos_theta, const float *g, size_t n, float *out);
} VptVolumeFns;

/* Which arms of the volume-forward form a render went through. */
typedef struct VptCoverage {
  uint64_t phase_vertices;      /* scatters inside a region */
  uint64_t phase_nee;           /* ... whose volume_nee sent a shadow ray */
  uint64_t depth_walks;         /* transmittance walks of a depth-exhausted segment */
  uint64_t medium_walks;        /* segments walked while the ray carried an interior medium */
  uint64_t phase_prev_hits;     /* bounce_emission_weight with a Phase previous vertex */
  uint64_t phase_prev_escapes;  /* escaped_emission competing with a Phase previous vertex */
} VptCoverage;

typedef struct VptJob {
  OraRenderJob job;            /* `forward` is ignored: this integrator has the forward form only */
  const VptVolumeFns *volumes; /* NULL: no aggregate bound */
  /* NULL, or light_sample / light_pdf / light_escaped of an OraSeamHooks (the other members are not read): lights the
   * oracle's light functions do not know (a mapped dome) go through somebody else's */
  const OraSeamHooks *light_hooks;
} VptJob;

/* domain.rng(): the seed of a walk drawn off a domain — the word ora_draw_rnd1 hashes (pattern and sample index), so the
 * walk's first number is the domain's draw_rnd1 (kernels/qmc.hip.h, rng_seed). */
static uint32_t rng_seed(OraSampler s) { return s.pattern ^ (s.index * 0x9e3779b9u + 0x7f4a7c15u); }
static int samples_lights(int s) { return s != ORA_STRATEGY_BSDF; } /* tracer.rs:79-81 */
static void put3(float *d, v3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }

static int l_sample(const VptJob *J, const OraLight *l, v3 from, float u, float v, OraLightSample *out) {
  if (!J->light_hooks || !J->light_hooks->light_sample) return ora_light_sample_li(l, from, u, v, out);
  float f[3]; put3(f, from);
  return J->light_hooks->light_sample(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), f, u, v, out);
}
static float l_pdf(const VptJob *J, const OraLight *l, v3 from, v3 point) {
  if (!J->light_hooks || !J->light_hooks->light_pdf) return ora_light_pdf_at_point(l, from, point);
  float f[3], p[3]; put3(f, from); put3(p, point);
  return J->light_hooks->light_pdf(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), f, p);
}
static int l_escaped(const VptJob *J, const OraLight *l, v3 direction, v3 *emitted, float *pdf) {
  if (!J->light_hooks || !J->light_hooks->light_escaped) return ora_light_escaped(l, direction, emitted, pdf);
  float d[3], e[3] = {0.0f, 0.0f, 0.0f}; put3(d, direction);
  int some = J->light_hooks->light_escaped(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), d, e, pdf);
  *emitted = v3_new(e[0], e[1], e[2]);
  return some;
}

/* ---- the aggregate, one query at a time ---- */
static CrtVolumeQuery vquery(const OraRay *ray, float t_eps, float t_max, uint32_t seed) {
  CrtVolumeQuery q;
  memset(&q, 0, sizeof q);
  put3(q.origin, ray->origin); put3(q.direction, ray->dir);
  q.t_eps = t_eps; q.t_max = t_max; q.seed = seed;
  return q;
}
/* does any region have an active interval on the segment (Volumes::active_intervals is not empty) */
static int vol_active(const VptJob *J, const OraRay *ray, float t_eps, float t_max) {
  if (!J->volumes) return 0;
  CrtVolumeQuery q = vquery(ray, t_eps, t_max, 0u);
  float out[18];
  uint32_t mask;
  J->volumes->intervals_n(J->volumes->image, &q, 1, out);
  memcpy(&mask, &out[0], 4);
  return mask != 0u;
}
static v3 vol_transmittance(const VptJob *J, const OraRay *ray, float t_eps, float t_max, uint32_t seed) {
  CrtVolumeQuery q = vquery(ray, t_eps, t_max, seed);
  CrtVolumeTransmittance t;
  J->volumes->transmittance_n(J->volumes->image, &q, 1, &t);
  return v3_new(t.transmittance[0], t.transmittance[1], t.transmittance[2]); /* all zero on CRT_VOLUME_STEP_LIMIT */
}
/* PhaseMix::pdf (volume.rs:319-324) of a scatter's lobes, unclamped */
static float phase_mix_pdf(const VptJob *J, const CrtVolumeEvent *E, float cos_theta) {
  float sum = 0.0f;
  for (uint32_t k = 0; k < E->n_lobes; k++) {
    float hg;
    J->volumes->hg_phase_n(&cos_theta, &E->lobes[k][1], 1, &hg);
    sum += E->lobes[k][0] * hg;
  }
  return sum;
}

/* rt_world.rs:191-196 */
typedef struct { OraHitRecord rec; const OraMaterial *mat; uint32_t geom_id, prim_id; } WorldHit;

static int world_intersect(const OraRenderJob *job, const OraRay *ray, float t_min, float t_max, WorldHit *out) {
  OraRayHit h; /* rt_world.rs:207-232 */
  if (!ora_intersect(job->scene, ray, t_min, t_max, &h)) return 0;
  out->rec.p = v3_add(ray->origin, v3_scale(ray->dir, h.t));
  out->rec.normal = h.normal;
  out->rec.t = h.t;
  out->rec.front_face = h.front_face;
  out->mat = &job->materials[h.geom_id];
  out->geom_id = h.geom_id;
  out->prim_id = h.prim_id;
  return 1;
}

/* tracer.rs:899-906: PrevVertex. phase: PrevVertex::Phase{p, pdf} — valid, never delta, always evaluable; rec.p = p. */
typedef struct { int valid, phase; v3 ray_dir; OraHitRecord rec; const OraMaterial *mat; v3 dir; float pdf; int delta; } PrevVertex;

static const OraLight *find_by_geom(const OraRenderJob *job, uint32_t geom_id) { /* light.rs:436-440 */
  for (uint32_t i = 0; i < job->n_lights; i++)
    if (job->lights[i].geom_id == geom_id) return &job->lights[i];
  return NULL;
}

static float bounce_emission_weight(const VptJob *J, const PrevVertex *p, const WorldHit *hit, VptCoverage *cov) { /* tracer.rs:930-953 */
  const OraRenderJob *job = &J->job;
  if (p->phase) {
    cov->phase_prev_hits++;
  } else {
    v3 val; float pdf;
    if (p->delta || !ora_mat_eval(p->mat, p->ray_dir, &p->rec, p->dir, &val, &pdf)) return 1.0f;
  }
  const OraLight *light = find_by_geom(job, hit->geom_id);
  if (!light) return 1.0f;
  float light_pdf = ora_max(l_pdf(J, light, p->rec.p, hit->rec.p) / (float)job->n_lights, 1e-6f);
  return ora_bounce_weight(job->strategy, p->pdf, light_pdf);
}

static v3 sky(v3 unit_direction) { /* tracer.rs:1334-1336 */
  float t = 0.5f * (unit_direction.y + 1.0f);
  return v3_add(v3_scale(v3_new(1.0f, 1.0f, 1.0f), 1.0f - t), v3_scale(v3_new(0.5f, 0.7f, 1.0f), t));
}

/* What an unoccluded shadow request pays: its contribution, times the segment's transmittance where a region is crossed
 * (the last operation on it; seed K_NEE_SHADOW off the vertex domain). */
static v3 shadow_payout(const VptJob *J, const OraRay *shadow_ray, float t_max, OraSampler v, v3 contribution) {
  if (!vol_active(J, shadow_ray, 0.001f, t_max)) return contribution;
  return v3_mul(contribution, vol_transmittance(J, shadow_ray, 0.001f, t_max, rng_seed(ora_new_domain(v, K_NEE_SHADOW))));
}

static v3 trace_path(const VptJob *J, const OraRay *r, OraSampler sampler, OraRayStats *stats, VptCoverage *cov) {
  const OraRenderJob *job = &J->job;
  OraSampler path = ora_new_domain(sampler, K_PATH);
  uint32_t n_rec = 0;
  OraRay ray = *r;
  int32_t remaining = (int32_t)job->max_depth;
  PrevVertex prev; memset(&prev, 0, sizeof prev);
  v3 beta = v3_splat(1.0f);
  v3 L = v3_splat(0.0f);
  const v3 one = v3_splat(1.0f);
  OraMedium med; int has_med = 0;
  memset(&med, 0, sizeof med);

  for (;;) {
    OraSampler v = ora_new_domain(path, (int)n_rec);
    const uint32_t vol_seed = rng_seed(ora_new_domain(v, K_VOLUME));
    if (remaining <= 0) { /* tracer.rs:1123-1149 */
      stats->ended_depth++;
      if (prev.valid) {
        stats->closest_hit++;
        WorldHit hit;
        if (world_intersect(job, &ray, 0.001f, ORA_INF, &hit)) {
          if (vol_active(J, &ray, 0.001f, hit.rec.t)) { /* tracer.rs:1138-1141, volume-forward: into beta first */
            beta = v3_mul(beta, vol_transmittance(J, &ray, 0.001f, hit.rec.t, vol_seed));
            cov->depth_walks++;
          }
          float cos_o = ora_abs(v3_dot(v3_normalize(ray.dir), hit.rec.normal));
          v3 emitted = ora_mat_emitted_directional(hit.mat, cos_o);
          if (v3_len2(emitted) > 0.0f) {
            if (has_med) emitted = v3_mul(emitted, ora_medium_transmittance(&med, hit.rec.t));
            float w = bounce_emission_weight(J, &prev, &hit, cov);
            L = v3_add(L, v3_mul(beta, v3_scale(emitted, w)));
          }
        }
      }
      break;
    }

    stats->closest_hit++;
    WorldHit hit;
    int has_hit = world_intersect(job, &ray, 0.001f, ORA_INF, &hit); /* tracer.rs:1152 */
    const float t_surf = has_hit ? hit.rec.t : ORA_INF;
    float t_med = ORA_INF; /* tracer.rs:1159-1165 */
    if (has_med && ora_medium_is_scattering(&med)) {
      float sigma_t_max = ora_max(ora_medium_sigma_t_max(&med), 1e-4f);
      t_med = -(ora_logf(ora_draw_rnd1(ora_new_domain(v, K_MEDIUM)))) / sigma_t_max;
    }

    /* === volume regions on the segment (tracer.rs:1167-1254), volume-forward === */
    const float t_end = t_med < t_surf ? t_med : t_surf;
    if (vol_active(J, &ray, 0.001f, t_end)) {
      float ps[4];
      ora_draw_sample4(ora_new_domain(v, K_PHASE), ps);
      CrtVolumeQuery q = vquery(&ray, 0.001f, t_end, vol_seed);
      CrtVolumeEvent E;
      J->volumes->sample_n(J->volumes->image, &q, ps, 1, &E); /* a CRT_VOLUME_STEP_LIMIT walk: weight 0, emitted 0 */
      L = v3_add(L, v3_mul(beta, v3_new(E.emitted[0], E.emitted[1], E.emitted[2])));
      beta = v3_mul(beta, v3_new(E.weight[0], E.weight[1], E.weight[2]));
      if (has_med) cov->medium_walks++;
      if (E.kind == CRT_VOLUME_SCATTER) { /* the phase vertex (tracer.rs:1192-1249) */
        cov->phase_vertices++;
        const v3 wi = v3_normalize(ray.dir);
        const v3 p = v3_new(E.p[0], E.p[1], E.p[2]);
        const v3 dir = v3_new(E.dir[0], E.dir[1], E.dir[2]);
        const float phase_pdf = E.pdf;
        /* volume_nee (tracer.rs:1040-1076) */
        if (samples_lights(job->strategy) && job->n_lights > 0) {
          float nee_s[4];
          ora_draw_sample4(ora_new_domain(v, K_NEE), nee_s);
          size_t li = (size_t)(nee_s[0] * (float)job->n_lights);
          if (li > job->n_lights - 1) li = job->n_lights - 1;
          const OraLight *light = &job->lights[li];
          OraLightSample ls;
          if (l_sample(J, light, p, nee_s[1], nee_s[2], &ls)) {
            OraRay shadow_ray = {p, ls.direction, ray.time, ORA_MASK_SHADOW};
            stats->shadow_rays++;
            cov->phase_nee++;
            const float t_max = ls.distance - 0.001f;
            int occluded = ora_occluded(job->scene, &shadow_ray, 0.001f, t_max);
            const float phase_val = phase_mix_pdf(J, &E, v3_dot(wi, ls.direction));
            const float light_pdf = ora_max(ls.pdf / (float)job->n_lights, 1e-6f);
            const v3 c = v3_divs(v3_scale(v3_scale(ls.radiance, phase_val), ora_light_weight(job->strategy, light_pdf, phase_val)), light_pdf);
            if (!occluded) L = v3_add(L, shadow_payout(J, &shadow_ray, t_max, v, v3_mul(beta, c)));
          }
        }
        int survived = 1;
        if (n_rec >= RR_START_BOUNCE) {
          stats->rr_tested++;
          float p_survive = ora_clamp(v3_max_elem(beta), RR_MIN_PROB, 1.0f);
          if (p_survive < 1.0f) {
            if (ora_draw_rnd1(ora_new_domain(v, K_RR)) >= p_survive) {
              survived = 0;
              stats->rr_killed++;
            } else {
              beta = v3_divs(beta, p_survive);
            }
          }
        }
        stats->vertices++;
        n_rec++;
        if (!survived) break;
        ray.origin = p; ray.dir = dir; ray.mask = ORA_MASK_INDIRECT; /* same medium, time kept */
        remaining -= 1;
        memset(&prev, 0, sizeof prev);
        prev.valid = 1; prev.phase = 1; prev.rec.p = p; prev.pdf = phase_pdf; prev.delta = 0;
        continue;
      }
    }

    if (t_med < t_surf) { /* === carried-medium scatter vertex (tracer.rs:1256-1319) === */
      float sigma_bar = ora_max(ora_medium_sigma_t_max(&med), 1e-4f);
      v3 pos = v3_add(ray.origin, v3_scale(ray.dir, t_med));
      float phase_uv[4];
      ora_draw_sample4(ora_new_domain(v, K_PHASE), phase_uv);
      v3 dir = ora_sample_henyey_greenstein(v3_normalize(ray.dir), med.g, phase_uv[0], phase_uv[1]);
      v3 e = v3_scale(v3_sub(v3_splat(sigma_bar), v3_add(med.sigma_a, med.sigma_s)), t_med);
      v3 factor = v3_mul(v3_divs(med.sigma_s, sigma_bar), v3_new(ora_expf(e.x), ora_expf(e.y), ora_expf(e.z)));
      beta = v3_mul(beta, v3_mul(one, factor));
      int survived = 1;
      if (n_rec >= RR_START_BOUNCE) {
        stats->rr_tested++;
        float p_survive = ora_clamp(v3_max_elem(beta), RR_MIN_PROB, 1.0f);
        if (p_survive < 1.0f) {
          if (ora_draw_rnd1(ora_new_domain(v, K_RR)) >= p_survive) {
            survived = 0;
            stats->rr_killed++;
          } else {
            beta = v3_divs(beta, p_survive);
          }
        }
      }
      stats->vertices++;
      n_rec++;
      if (!survived) break;
      ray.origin = pos; ray.dir = dir; ray.mask = ORA_MASK_INDIRECT;
      remaining -= 1;
      prev.valid = 0; prev.phase = 0;
      continue;
    }
    if (!has_hit) { /* tracer.rs:1321-1342 with escaped_emission (:966-1009) */
      stats->ended_escaped++;
      v3 unit_direction = v3_normalize(ray.dir);
      v3 background = v3_splat(0.0f);
      int covered = 0;
      if (job->n_lights > 0) {
        int competing = prev.valid && !prev.delta;
        if (competing && prev.phase) cov->phase_prev_escapes++;
        float n_lights = (float)job->n_lights;
        for (uint32_t k = 0; k < job->n_lights; k++) {
          v3 emitted; float pdf;
          if (!l_escaped(J, &job->lights[k], unit_direction, &emitted, &pdf)) continue;
          covered = 1;
          float weight = 1.0f;
          if (competing && samples_lights(job->strategy)) {
            float light_pdf = ora_max(pdf / n_lights, 1e-6f);
            weight = ora_bounce_weight(job->strategy, prev.pdf, light_pdf);
          }
          background = v3_add(background, v3_scale(emitted, weight));
        }
      }
      if (!covered) background = v3_add(background, sky(unit_direction));
      L = v3_add(L, v3_mul(beta, background));
      break;
    }
    const OraHitRecord rec = hit.rec;
    const OraMaterial *mat = hit.mat;
    v3 atten = one; /* tracer.rs:1352-1361; segment transmittance of the regions has entered beta already */
    if (has_med) {
      if (ora_medium_is_scattering(&med)) {
        float sigma_bar = ora_max(ora_medium_sigma_t_max(&med), 1e-4f);
        v3 e = v3_scale(v3_sub(v3_splat(sigma_bar), v3_add(med.sigma_a, med.sigma_s)), rec.t);
        atten = v3_mul(one, v3_new(ora_expf(e.x), ora_expf(e.y), ora_expf(e.z)));
      } else {
        atten = v3_mul(one, ora_medium_transmittance(&med, rec.t));
      }
    }

    float cos_o = ora_abs(v3_dot(v3_normalize(ray.dir), rec.normal)); /* tracer.rs:1369-1381 */
    v3 emitted = ora_mat_emitted_directional(mat, cos_o);
    v3 emit_here = v3_splat(0.0f);
    if (prev.valid) {
      if (v3_len2(emitted) > 0.0f) {
        float w = bounce_emission_weight(J, &prev, &hit, cov);
        L = v3_add(L, v3_mul(beta, v3_scale(v3_mul(atten, emitted), w)));
      }
    } else {
      emit_here = emitted;
    }
    const v3 ba = v3_mul(beta, atten);
    L = v3_add(L, v3_mul(ba, emit_here));

    /* === 1. NEE (tracer.rs:1394-1445): what the deferred shadow test pays out === */
    if (samples_lights(job->strategy) && job->n_lights > 0) {
      float nee_s[4];
      ora_draw_sample4(ora_new_domain(v, K_NEE), nee_s);
      size_t li = (size_t)(nee_s[0] * (float)job->n_lights); /* light.rs:421-429 */
      if (li > job->n_lights - 1) li = job->n_lights - 1;
      const OraLight *light = &job->lights[li];
      OraLightSample ls;
      if (l_sample(J, light, rec.p, nee_s[1], nee_s[2], &ls)) {
        float n_lights = (float)job->n_lights;
        OraRay shadow_ray = {rec.p, ls.direction, ray.time, ORA_MASK_SHADOW};
        stats->shadow_rays++; /* tracer.rs:1026 */
        const float t_max = ls.distance - 0.001f;
        int occluded = ora_occluded(job->scene, &shadow_ray, 0.001f, t_max);
        if (!occluded) {
          float cosine = ora_abs(v3_dot(rec.normal, ls.direction));
          float light_pdf = ora_max(ls.pdf / n_lights, 1e-6f);
          v3 brdf_value; float brdf_pdf;
          v3 nee = v3_splat(0.0f);
          if (ora_mat_eval(mat, ray.dir, &rec, ls.direction, &brdf_value, &brdf_pdf)) {
            float weight = ora_light_weight(job->strategy, light_pdf, brdf_pdf);
            v3 c = v3_scale(v3_mul(ls.radiance, brdf_value), cosine);
            c = v3_mul(c, one);
            nee = v3_add(nee, v3_divs(v3_scale(c, weight), light_pdf));
          }
          L = v3_add(L, shadow_payout(J, &shadow_ray, t_max, v, v3_mul(ba, nee)));
        }
      }
    }

    /* === 2. bounce (tracer.rs:1459-1523) === */
    OraScatter sample;
    if (ora_mat_scatter(mat, ray.dir, &rec, ora_new_domain(v, K_BSDF), &sample)) {
      v3 dir = v3_normalize(sample.dir);
      float cosine = sample.delta ? 1.0f : ora_abs(v3_dot(rec.normal, dir));
      v3 factor = v3_divs(v3_scale(sample.value, cosine), sample.pdf);
      beta = v3_mul(beta, v3_mul(atten, factor));
      int survived = 1;
      if (n_rec >= RR_START_BOUNCE) {
        stats->rr_tested++;
        float p_survive = ora_clamp(v3_max_elem(beta), RR_MIN_PROB, 1.0f);
        if (p_survive < 1.0f) {
          if (ora_draw_rnd1(ora_new_domain(v, K_RR)) >= p_survive) {
            survived = 0;
            stats->rr_killed++;
          } else {
            beta = v3_divs(beta, p_survive);
          }
        }
      }
      if (survived) {
        prev.valid = 1; prev.phase = 0; prev.ray_dir = ray.dir; prev.rec = rec; prev.mat = mat; prev.dir = dir; prev.pdf = sample.pdf;
        prev.delta = sample.delta;
        stats->vertices++;
        n_rec++;
        ray.origin = sample.origin; ray.dir = sample.dir; ray.mask = ORA_MASK_INDIRECT; /* time kept */
        has_med = sample.medium ? ora_interior_medium(mat, &med) : 0;
        remaining -= 1;
        continue;
      }
    }
    stats->vertices++;
    n_rec++;
    break;
  }
  return L;
}

static float luminance(v3 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; } /* guiding/mod.rs:18-20 */

static v3 camera_sample(const VptJob *J, uint32_t i, uint32_t j, uint32_t sample, OraRayStats *stats, VptCoverage *cov,
                        float *w_out) { /* tracer.rs:559-598 */
  const OraRenderJob *job = &J->job;
  int tile = (int)(i >> 8) + (int)(j >> 8) * 4096; /* tracer.rs:543 */
  OraSampler root = ora_new_domain(ora_sampler_new((int)i, (int)j, job->frame, (int)sample), tile);
  float cam[4];
  ora_draw_sample4(ora_new_domain(root, K_CAMERA), cam);
  float fx, wx, fy, wy;
  ora_filter_sample(job->filter_kind, job->filter_radius, cam[0], &fx, &wx);
  ora_filter_sample(job->filter_kind, job->filter_radius, cam[1], &fy, &wy);
  float u = ((float)i + fx) / (float)job->width;
  float v = ((float)j + fy) / (float)job->height;
  float time = 0.0f;
  if (ora_has_motion(job->scene)) { /* tracer.rs:579-583 */
    float t4[4];
    ora_draw_sample4(ora_new_domain(root, K_TIME), t4);
    time = t4[0];
  }
  OraRay r;
  ora_camera_get_ray(&job->camera, u, v, cam[2], cam[3], time, &r);
  stats->camera_rays++;
  v3 color = trace_path(J, &r, root, stats, cov);
  *w_out = wx * wy;
  return color;
}

/* One camera sample of one pixel: radiance before the filter weight — ora_render_sample's counterpart. */
void vpt_render_sample(const VptJob *J, uint32_t i, uint32_t j, uint32_t sample, float rgb[3], OraRayStats *stats,
                       VptCoverage *cov) {
  float w;
  v3 c = camera_sample(J, i, j, sample, stats, cov, &w);
  rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
}

static uint32_t render_pixel(const VptJob *J, uint32_t i, uint32_t j, float rgb[3], OraRayStats *stats, VptCoverage *cov) { /* tracer.rs:515-636 */
  const OraRenderJob *job = &J->job;
  v3 sum = v3_splat(0.0f);
  float weight_sum = 0.0f;
  double lum_sum = 0.0, lum_sq = 0.0;
  double threshold = (double)job->variance_threshold;
  uint32_t min_spp = job->min_spp > 2 ? job->min_spp : 2;
  uint32_t taken = 0;
  for (uint32_t sample = 0; sample < job->spp; sample++) {
    float w = 0.0f;
    v3 radiance = camera_sample(J, i, j, sample, stats, cov, &w);
    v3 color = v3_scale(radiance, w);
    sum = v3_add(sum, color);
    weight_sum += w;
    double lum = (double)luminance(color);
    lum_sum += lum;
    lum_sq += lum * lum;
    taken = sample + 1;
    if (threshold > 0.0 && taken >= min_spp && taken % 4 == 0) { /* tracer.rs:609-617 */
      double n = (double)taken;
      double var_of_mean = (lum_sq - lum_sum * lum_sum / n) / (n - 1.0) / n;
      if (!(var_of_mean > 0.0)) var_of_mean = 0.0;
      double mean = lum_sum / n;
      if (!(mean > 1e-4)) mean = 1e-4;
      if (sqrt(var_of_mean) / mean < threshold) break;
    }
  }
  v3 mean = weight_sum > 0.0f ? v3_divs(sum, weight_sum) : v3_divs(sum, (float)taken);
  rgb[0] = mean.x; rgb[1] = mean.y; rgb[2] = mean.z;
  return taken;
}

typedef struct {
  const VptJob *J; float *rgb; uint32_t *counts; OraRayStats stats; VptCoverage cov;
  uint32_t *next_row; pthread_mutex_t *mu;
} Worker;

static void *worker_main(void *arg) {
  Worker *w = (Worker *)arg;
  const OraRenderJob *job = &w->J->job;
  for (;;) {
    pthread_mutex_lock(w->mu);
    uint32_t j = (*w->next_row)++;
    pthread_mutex_unlock(w->mu);
    if (j >= job->height) break;
    for (uint32_t i = 0; i < job->width; i++) {
      const size_t at = (size_t)j * job->width + i;
      const uint32_t taken = render_pixel(w->J, i, j, w->rgb + 3 * at, &w->stats, &w->cov);
      if (w->counts) w->counts[at] = taken;
    }
  }
  return NULL;
}

/* The frame: rgb (width * height * 3, buffer order as ora_render), per-pixel sample counts (may be NULL), the eight
 * RayStats and the coverage counters. Pixels are independent (tracer.rs:543, :559-560): rows go to n_threads workers.
 * With Python callbacks in the function table or the light hooks, n_threads = 1. */
void vpt_render(const VptJob *J, float *rgb, uint32_t *counts, OraRayStats *stats, VptCoverage *cov, int n_threads) {
  if (n_threads < 1) n_threads = 1;
  uint32_t next = 0;
  pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
  Worker *ws = (Worker *)calloc((size_t)n_threads, sizeof(Worker));
  pthread_t *th = (pthread_t *)calloc((size_t)n_threads, sizeof(pthread_t));
  for (int k = 0; k < n_threads; k++) {
    ws[k].J = J; ws[k].rgb = rgb; ws[k].counts = counts; ws[k].next_row = &next; ws[k].mu = &mu;
    if (n_threads > 1) pthread_create(&th[k], NULL, worker_main, &ws[k]);
    else worker_main(&ws[k]);
  }
  OraRayStats total; memset(&total, 0, sizeof total);
  VptCoverage ctot; memset(&ctot, 0, sizeof ctot);
  for (int k = 0; k < n_threads; k++) {
    if (n_threads > 1) pthread_join(th[k], NULL);
    const OraRayStats *b = &ws[k].stats;
    total.camera_rays += b->camera_rays; total.closest_hit += b->closest_hit; total.shadow_rays += b->shadow_rays;
    total.vertices += b->vertices; total.rr_tested += b->rr_tested; total.rr_killed += b->rr_killed;
    total.ended_escaped += b->ended_escaped; total.ended_depth += b->ended_depth;
    const VptCoverage *c = &ws[k].cov;
    ctot.phase_vertices += c->phase_vertices; ctot.phase_nee += c->phase_nee; ctot.depth_walks += c->depth_walks;
    ctot.medium_walks += c->medium_walks; ctot.phase_prev_hits += c->phase_prev_hits; ctot.phase_prev_escapes += c->phase_prev_escapes;
  }
  if (stats) *stats = total;
  if (cov) *cov = ctot;
  free(ws); free(th);
}
