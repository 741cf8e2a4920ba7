/* TEST INFRASTRUCTURE ONLY: a guiding-aware forward integrator, the truth the wavefront renderer's guided renders are
 * compared with bit for bit (tests/test_guided_render.py, tests/test_gpu_guided_render.py).
 *
 * The oracle (oracle/ora_pt.c) knows no guiding field. This file restates camera_sample, render_pixel (adaptive rule
 * included) and trace_path (tracer.rs:515-636, :1086-1558) in the oracle's FORWARD form, as tests/volume_pt/volume_pt.c
 * does — without volumes — on the oracle's exported functions, and adds the two steps of the guided pass
 * (render_pass(.., Some(&GuidingContext{field, training: false}))), both at vertices that have a previous vertex
 * (tracer.rs:1386):
 *   - the bounce: sample_bounce_direction (tracer.rs:777-826) in the place of scatter_importance;
 *   - the bounce pdf inside the NEE MIS weight (tracer.rs:1432-1440): the guide / BSDF mixture where the field is trained.
 * With no table bound, or an untrained field, it is the oracle's forward mode operation for operation
 * (test_guided_render.py pins that on three scenes).
 *
 * The field is reached through a function table (GptGuideFns) of two calls with n = 1: the guided bounce, with the
 * signature of host_guide_scatter_n, and the pdf, with the signature of host_guide_pdf_n (it also answers `trained`) —
 * tests/host_shade/guiding_host.cpp, the device source compiled for the host, itself pinned to the numpy restatement
 * tests/guiding_ref.py. The table may instead hold Python callbacks into guiding_ref.Field composed with the oracle's
 * scatter / eval drivers (one thread then).
 *
 * -DGPT_PLAIN_NEE_PDF builds the WRONG variant: the plain BSDF pdf in the light weight beside a guided bounce. One test
 * uses it, to show that the unbiasedness bound can fail.
 *
 * Built at test time by tests/guided_pt/__init__.py against oracle/_build/liboracle.so. */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/crt_guiding.h"
#include "../../oracle/ora_pt.h"

enum { K_CAMERA = 0, K_PATH = 1, K_TIME = 2 };                                                                  /* tracer.rs:20-22 */
enum { K_NEE = 0, K_NEE_SHADOW = 1, K_BSDF = 2, K_GUIDE = 3, K_PHASE = 4, K_RR = 5, K_MEDIUM = 6, K_VOLUME = 7 }; /* :23-30 */
#define RR_START_BOUNCE 3 /* tracer.rs:46 */
#define RR_MIN_PROB 0.05f /* tracer.rs:47 */

typedef struct GptGuideFns {
  const void *image; /* handed back as the first argument: the field's byte image, or any context */
  /* sample_bounce_direction off the VERTEX domain (query.sampler_*): CrtScatterSample, flags bits 0-3 as
   * crt_material_scatter_guided_n documents them */
  void (*scatter_n)(const void *image, const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *q, size_t n, CrtScatterSample *out);
  /* GuidingField::pdf(pos, dir) and trained_at(pos) */
  void (*pdf_n)(const void *image, const CrtGuidingQuery *q, size_t n, CrtGuidingResult *out);
  float alpha; /* guide_prob: read for the coverage record only (which exit a trained bounce took) */
} GptGuideFns;

/* Which arms of the guided pass a render went through. */
typedef struct GptCoverage {
  uint64_t exits[5];             /* the bounce: untrained, guide, guide_fallback, bsdf_delta, bsdf_continuous */
  uint64_t nee_mixture;          /* NEE weights that used the mixture pdf */
  uint64_t nee_trained_no_eval;  /* NEE at a trained vertex whose eval was None */
  uint64_t primary_unguided;     /* camera vertices, left unguided */
  uint64_t post_medium_unguided; /* vertices behind an interior-medium scatter, left unguided */
} GptCoverage;

typedef struct GptJob {
  OraRenderJob job;          /* `forward` is ignored: this integrator has the forward form only */
  const GptGuideFns *guide;  /* NULL: no field bound */
  /* NULL, or light_sample / light_pdf / light_escaped of an OraSeamHooks (the other members are not read): lights the
   * oracle's light functions do not know (a mapped dome) go through somebody else's */
  const OraSeamHooks *light_hooks;
} GptJob;

static int samples_lights(int s) { return s != ORA_STRATEGY_BSDF; } /* tracer.rs:79-81 */
static void put3(float *d, v3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }

static int l_sample(const GptJob *J, const OraLight *l, v3 from, float u, float v, OraLightSample *out) {
  if (!J->light_hooks || !J->light_hooks->light_sample) return ora_light_sample_li(l, from, u, v, out);
  float f[3]; put3(f, from);
  return J->light_hooks->light_sample(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), f, u, v, out);
}
static float l_pdf(const GptJob *J, const OraLight *l, v3 from, v3 point) {
  if (!J->light_hooks || !J->light_hooks->light_pdf) return ora_light_pdf_at_point(l, from, point);
  float f[3], p[3]; put3(f, from); put3(p, point);
  return J->light_hooks->light_pdf(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), f, p);
}
static int l_escaped(const GptJob *J, const OraLight *l, v3 direction, v3 *emitted, float *pdf) {
  if (!J->light_hooks || !J->light_hooks->light_escaped) return ora_light_escaped(l, direction, emitted, pdf);
  float d[3], e[3] = {0.0f, 0.0f, 0.0f}; put3(d, direction);
  int some = J->light_hooks->light_escaped(J->light_hooks->ctx, (uint32_t)(l - J->job.lights), d, e, pdf);
  *emitted = v3_new(e[0], e[1], e[2]);
  return some;
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

/* tracer.rs:899-906: PrevBounce. pdf is the density the bounce was drawn with: the mixture at a guided vertex. */
typedef struct { int valid; v3 ray_dir; OraHitRecord rec; const OraMaterial *mat; v3 dir; float pdf; int delta; } PrevVertex;

static const OraLight *find_by_geom(const OraRenderJob *job, uint32_t geom_id) { /* light.rs:436-440 */
  for (uint32_t i = 0; i < job->n_lights; i++)
    if (job->lights[i].geom_id == geom_id) return &job->lights[i];
  return NULL;
}

static float bounce_emission_weight(const GptJob *J, const PrevVertex *p, const WorldHit *hit) { /* tracer.rs:930-953 */
  const OraRenderJob *job = &J->job;
  v3 val; float pdf;
  if (p->delta || !ora_mat_eval(p->mat, p->ray_dir, &p->rec, p->dir, &val, &pdf)) return 1.0f;
  const OraLight *light = find_by_geom(job, hit->geom_id);
  if (!light) return 1.0f;
  float light_pdf = ora_max(l_pdf(J, light, p->rec.p, hit->rec.p) / (float)job->n_lights, 1e-6f);
  return ora_bounce_weight(job->strategy, p->pdf, light_pdf);
}

static v3 sky(v3 unit_direction) { /* tracer.rs:1334-1336 */
  float t = 0.5f * (unit_direction.y + 1.0f);
  return v3_add(v3_scale(v3_new(1.0f, 1.0f, 1.0f), 1.0f - t), v3_scale(v3_new(0.5f, 0.7f, 1.0f), t));
}

/* ---- the field, one query at a time ---- */
/* GuidingField::pdf(p, dir); *trained = trained_at(p) */
static float guide_pdf(const GptJob *J, v3 p, v3 dir, int *trained) {
  CrtGuidingQuery q;
  CrtGuidingResult r;
  memset(&q, 0, sizeof q); memset(&r, 0, sizeof r);
  put3(q.pos, p); put3(q.dir, dir);
  J->guide->pdf_n(J->guide->image, &q, 1, &r);
  *trained = r.trained != 0;
  return r.pdf;
}
/* sample_bounce_direction(ray, rec, mat, Some(guiding), v): 1 and *out, or 0 for None; *flags: bit 2 trained, bit 3 from the guide */
static int guided_bounce(const GptJob *J, const OraRay *ray, const OraHitRecord *rec, uint32_t geom_id, OraSampler v, OraScatter *out,
                         uint32_t *flags) {
  CrtShadeQuery q;
  CrtScatterSample s;
  memset(&q, 0, sizeof q); memset(&s, 0, sizeof s);
  put3(q.ray_dir, ray->dir); q.material = geom_id;
  put3(q.p, rec->p); q.t = rec->t;
  put3(q.normal, rec->normal); q.front_face = rec->front_face ? 1u : 0u;
  q.sampler_pattern = v.pattern; q.sampler_index = v.index;
  J->guide->scatter_n(J->guide->image, (const CrtMaterial *)J->job.materials, J->job.n_materials, &q, 1, &s);
  *flags = s.flags;
  if (!s.some) return 0;
  out->origin = v3_new(s.origin[0], s.origin[1], s.origin[2]);
  out->dir = v3_new(s.dir[0], s.dir[1], s.dir[2]);
  out->value = v3_new(s.value[0], s.value[1], s.value[2]);
  out->pdf = s.pdf;
  out->delta = (s.flags & 1u) != 0;
  out->medium = (s.flags & 2u) != 0;
  return 1;
}

static v3 trace_path(const GptJob *J, const OraRay *r, OraSampler sampler, OraRayStats *stats, GptCoverage *cov) {
  const OraRenderJob *job = &J->job;
  OraSampler path = ora_new_domain(sampler, K_PATH);
  uint32_t n_rec = 0;
  OraRay ray = *r;
  int32_t remaining = (int32_t)job->max_depth;
  PrevVertex prev; memset(&prev, 0, sizeof prev);
  int after_medium = 0; /* the previous vertex was an interior-medium scatter (prev = None behind it, tracer.rs:1317) */
  v3 beta = v3_splat(1.0f);
  v3 L = v3_splat(0.0f);
  const v3 one = v3_splat(1.0f);
  OraMedium med; int has_med = 0;
  memset(&med, 0, sizeof med);

  for (;;) {
    OraSampler v = ora_new_domain(path, (int)n_rec);
    if (remaining <= 0) { /* tracer.rs:1123-1149 */
      stats->ended_depth++;
      if (prev.valid) {
        stats->closest_hit++;
        WorldHit hit;
        if (world_intersect(job, &ray, 0.001f, ORA_INF, &hit)) {
          float cos_o = ora_abs(v3_dot(v3_normalize(ray.dir), hit.rec.normal));
          v3 emitted = ora_mat_emitted_directional(hit.mat, cos_o);
          if (v3_len2(emitted) > 0.0f) {
            if (has_med) emitted = v3_mul(emitted, ora_medium_transmittance(&med, hit.rec.t));
            float w = bounce_emission_weight(J, &prev, &hit);
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
      prev.valid = 0;
      after_medium = 1;
      continue;
    }
    if (!has_hit) { /* tracer.rs:1321-1342 with escaped_emission (:966-1009) */
      stats->ended_escaped++;
      v3 unit_direction = v3_normalize(ray.dir);
      v3 background = v3_splat(0.0f);
      int covered = 0;
      if (job->n_lights > 0) {
        int competing = prev.valid && !prev.delta;
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
    v3 atten = one; /* tracer.rs:1352-1361 */
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
        float w = bounce_emission_weight(J, &prev, &hit);
        L = v3_add(L, v3_mul(beta, v3_scale(v3_mul(atten, emitted), w)));
      }
    } else {
      emit_here = emitted;
    }
    const v3 ba = v3_mul(beta, atten);
    L = v3_add(L, v3_mul(ba, emit_here));

    /* tracer.rs:1386: secondary vertices only */
    const int guiding_here = J->guide != NULL && prev.valid;
    if (J->guide && !prev.valid) {
      if (after_medium) cov->post_medium_unguided++;
      else cov->primary_unguided++;
    }
    after_medium = 0;

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
          int trained = 0;
          float p_guide = 0.0f;
          if (guiding_here) p_guide = guide_pdf(J, rec.p, ls.direction, &trained);
          if (ora_mat_eval(mat, ray.dir, &rec, ls.direction, &brdf_value, &brdf_pdf)) {
            float bounce_pdf = brdf_pdf; /* tracer.rs:1432-1439 */
            if (trained) {
              const float alpha = J->guide->alpha;
              cov->nee_mixture++;
#ifndef GPT_PLAIN_NEE_PDF
              bounce_pdf = alpha * p_guide + (1.0f - alpha) * brdf_pdf;
#else
              (void)alpha; (void)p_guide; /* the WRONG variant: the plain BSDF pdf beside a guided bounce */
#endif
            }
            float weight = ora_light_weight(job->strategy, light_pdf, bounce_pdf);
            v3 c = v3_scale(v3_mul(ls.radiance, brdf_value), cosine);
            c = v3_mul(c, one);
            nee = v3_add(nee, v3_divs(v3_scale(c, weight), light_pdf));
          } else if (trained) {
            cov->nee_trained_no_eval++;
          }
          L = v3_add(L, v3_mul(ba, nee));
        }
      }
    }

    /* === 2. bounce (tracer.rs:1459-1523): sample_bounce_direction(.., guiding_here, v) === */
    OraScatter sample;
    int scattered;
    if (guiding_here) {
      uint32_t flags = 0;
      scattered = guided_bounce(J, &ray, &rec, hit.geom_id, v, &sample, &flags);
      int exit_taken = 0;
      if (flags & 4u) {
        float gs[4];
        ora_draw_sample4(ora_new_domain(v, K_GUIDE), gs);
        if (flags & 8u) exit_taken = 1;
        else if (gs[0] < J->guide->alpha) exit_taken = 2;
        else exit_taken = (scattered && sample.delta) ? 3 : 4;
      }
      cov->exits[exit_taken]++;
    } else {
      scattered = ora_mat_scatter(mat, ray.dir, &rec, ora_new_domain(v, K_BSDF), &sample);
    }
    if (scattered) {
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
        prev.valid = 1; prev.ray_dir = ray.dir; prev.rec = rec; prev.mat = mat; prev.dir = dir; prev.pdf = sample.pdf;
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

static v3 camera_sample(const GptJob *J, uint32_t i, uint32_t j, uint32_t sample, OraRayStats *stats, GptCoverage *cov,
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

static uint32_t render_pixel(const GptJob *J, uint32_t i, uint32_t j, float rgb[3], OraRayStats *stats, GptCoverage *cov) { /* tracer.rs:515-636 */
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
  const GptJob *J; float *rgb; uint32_t *counts; OraRayStats stats; GptCoverage cov;
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
void gpt_render(const GptJob *J, float *rgb, uint32_t *counts, OraRayStats *stats, GptCoverage *cov, int n_threads) {
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
  GptCoverage ctot; memset(&ctot, 0, sizeof ctot);
  for (int k = 0; k < n_threads; k++) {
    if (n_threads > 1) pthread_join(th[k], NULL);
    const OraRayStats *b = &ws[k].stats;
    total.camera_rays += b->camera_rays; total.closest_hit += b->closest_hit; total.shadow_rays += b->shadow_rays;
    total.vertices += b->vertices; total.rr_tested += b->rr_tested; total.rr_killed += b->rr_killed;
    total.ended_escaped += b->ended_escaped; total.ended_depth += b->ended_depth;
    const GptCoverage *c = &ws[k].cov;
    for (int e = 0; e < 5; e++) ctot.exits[e] += c->exits[e];
    ctot.nee_mixture += c->nee_mixture; ctot.nee_trained_no_eval += c->nee_trained_no_eval;
    ctot.primary_unguided += c->primary_unguided; ctot.post_medium_unguided += c->post_medium_unguided;
  }
  if (stats) *stats = total;
  if (cov) *cov = ctot;
  free(ws); free(th);
}
