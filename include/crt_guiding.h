/* libcrt_amd: the path guiding field — the GuidingField of crates/crust-core/src/guiding/{mod,dtree,sdtree,field}.rs
 * (Practical Path Guiding, Mueller et al. 2017: a binary spatial tree whose leaves own directional quadtrees) as a
 * host-built image and three batched device functions over it, for a host integrator that keeps its own trace_path on
 * crt_intersect_n / crt_occluded_n and the shading seam and wants to turn on crust:pathGuiding (tracer.rs:245-403).
 * A header of its own beside crt.h: crt.h's set of declarations is pinned (tests/test_volumes.py, tests/test_abi.py).
 * Exported by the same library; include it after, or instead of, crt.h. The wavefront renderer reads a
 * field only where one is bound to it (crt_render_guiding.h, crt_renderer_set_guiding: the guided pass; it trains nothing).
 *
 * The field lives on the host: crt_guiding_new / _update / _image / _stats touch no device. crt_guiding_update splats a
 * training pass in array order on one thread — the sums are f32 and the order is part of the result, as upstream's
 * (dtree.rs:60-61) — refines both trees operation for operation and flattens the result into one image; the device copy
 * is replaced at the next device call, after the library has waited for the device (hipDeviceSynchronize). The caller
 * must not have guiding launches in flight on other streams while it calls crt_guiding_update or crt_guiding_free.
 *
 * The batched calls follow the seam's conventions (crt.h): device pointers, a stream, no synchronisation; n == 0 is
 * CRT_OK, a NULL pointer CRT_ERR_BAD_ARG, no gfx950 device CRT_ERR_NO_DEVICE; arguments are checked before a device is
 * touched. Parity: DESIGN.md §2 (cos / sin / atan2 are the library's deterministic ones, so field bits are pinned
 * against a float32 restatement of the four files, tests/guiding_ref.py, and statistically against upstream's tests). */
#ifndef CRT_GUIDING_H
#define CRT_GUIDING_H

#include "crt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caps, not measurements: a device descent is a `for` loop whose trip count is the cap. DTree::refine (dtree.rs:226-275)
 * creates at most 1 / rho children per level, so one D-tree holds at most depth / rho = 32 Ki nodes (1 MB). */
#define CRT_GUIDING_MAX_DTREE_DEPTH   32u
#define CRT_GUIDING_MAX_SPATIAL_DEPTH 32u
#define CRT_GUIDING_MIN_RHO (1.0f / 1024.0f)

/* GuidingConfig, field.rs:13-41. 24 bytes */
typedef struct CrtGuidingConfig {
  uint32_t train_iterations; float guide_prob; float spatial_c; float dtree_rho;
  uint32_t dtree_max_depth; uint32_t spatial_max_depth;
} CrtGuidingConfig;
/* SampleData, field.rs:45-50. 32 bytes */
typedef struct CrtGuidingSample {
  float pos[3]; float radiance; float dir[3]; uint32_t _pad;
} CrtGuidingSample;
/* One query of crt_guiding_sample_n (pos, seed) or crt_guiding_pdf_n (pos, dir). 32 bytes */
typedef struct CrtGuidingQuery {
  float pos[3]; float seed_u;          /* sample: the 2-D seed (one QMC draw), dtree.rs:163 */
  float dir[3]; float seed_v;          /* pdf: the direction, field.rs:95                   */
} CrtGuidingQuery;
/* 32 bytes */
typedef struct CrtGuidingResult {
  float dir[3]; float pdf;             /* sample: Option<(dir, pdf)>, zeros for None | pdf: pdf only, dir = 0 */
  uint32_t some; uint32_t trained; uint32_t _pad[2];   /* trained = trained_at(pos) (field.rs:81-83), both calls; pdf: some = 1 */
} CrtGuidingResult;
/* Tallies of the field as it stands: spatial nodes, spatial leaves, the deepest leaf (the root is depth 0,
 * sdtree.rs:107-168), directional trees, their nodes in all, the deepest of them (DTree::depth, dtree.rs:280-291: a
 * single root is depth 1), and every sample crt_guiding_update has been handed (counted, whether or not it splat). */
typedef struct CrtGuidingStats { uint32_t s_nodes, s_leaves, s_depth, d_trees, d_nodes, d_depth; uint64_t recorded; } CrtGuidingStats;
typedef struct CrtGuiding CrtGuiding;

/* GuidingConfig::default, field.rs:30-41: 4, 0.5, 4000, 0.01, 20, 24. */
void crt_guiding_config_default(CrtGuidingConfig *cfg);
/* GuidingField::new, field.rs:63-72, the padding of the bounds included. Host only. NULL with the reason in
 * crt_last_error for: non-finite or inverted bounds; guide_prob not finite or outside (0, 1) (the mixture divides by
 * 1 - guide_prob; the clamp to [0.1, 0.9] is with_guiding's, tracer.rs:696-700, and belongs to the caller); spatial_c or
 * dtree_rho not finite or <= 0; dtree_rho < CRT_GUIDING_MIN_RHO; dtree_max_depth 0 or above its cap; spatial_max_depth
 * above its cap. */
CrtGuiding *crt_guiding_new(const float bmin[3], const float bmax[3], const CrtGuidingConfig *cfg);
/* Drops the field and its device copy (after waiting for the device). crt_guiding_free(NULL) is fine. */
void crt_guiding_free(CrtGuiding *g);
/* GuidingField::update, field.rs:101-112: SDTree::record per sample in array order (sdtree.rs:70-80; DTree::record,
 * dtree.rs:106-121), then SDTree::refine (sdtree.rs:86-168, the f64 threshold (c * sqrt(2^k)).max(1) as u64 included)
 * and DTree::refine (dtree.rs:226-275). host_samples is a HOST pointer: a training pass of a host integrator ends on the
 * host. Rebuilds the image; see the note on the device copy above. CRT_ERR_NO_MEMORY when an allocation fails. */
int crt_guiding_update(CrtGuiding *g, const CrtGuidingSample *host_samples, size_t n, uint32_t next_iteration);
/* The image the kernels read (host memory, valid until the next crt_guiding_update / _free): a 256-byte header, 16-byte
 * spatial nodes, 32-byte directional nodes, every array on a 256-byte boundary. Host only. */
int crt_guiding_image(const CrtGuiding *g, const void **image, size_t *bytes);
int crt_guiding_stats(const CrtGuiding *g, CrtGuidingStats *out);
/* GuidingField::sample, field.rs:88-91: SDTree::dtree_at (sdtree.rs:43-66), DTree::sample (dtree.rs:163-219),
 * canonical_to_dir (dtree.rs:38-43). */
int crt_guiding_sample_n(CrtGuiding *g, const CrtGuidingQuery *d_queries, size_t n, CrtGuidingResult *d_out, void *stream);
/* GuidingField::pdf, field.rs:95-97: dir_to_canonical (dtree.rs:30-35), DTree::pdf (dtree.rs:125-151). */
int crt_guiding_pdf_n(CrtGuiding *g, const CrtGuidingQuery *d_queries, size_t n, CrtGuidingResult *d_out, void *stream);
/* sample_bounce_direction, tracer.rs:777-826, on the device's own Material::scatter_importance / eval. The query's
 * sampler_pattern / sampler_index is the VERTEX domain v: the call derives new_domain(v, K_BSDF = 2) and
 * new_domain(v, K_GUIDE = 3) itself (crt_material_scatter_n is handed the BSDF domain). gs = draw_sample_f32::<4> of the
 * K_GUIDE domain: gs[0] is the alpha-coin, (gs[1], gs[2]) the seed. The five exits: untrained at rec.p — plain
 * scatter_importance; guide branch — value and BSDF pdf from eval, pdf = max(a * p_g + (1 - a) * p_b, 1e-4), the ray from
 * Material::make_ray (openpbr.rs:1186-1200; Emissive material.rs:79-81); guide branch falling back to scatter_importance
 * when sample or eval is None; BSDF branch, delta — value / (1 - a); BSDF branch, continuous — the mixture pdf, only
 * when eval(...).is_some(). Output flags: bits 0 and 1 as crt_material_scatter_n documents them; bit 2: the field was
 * trained at p; bit 3: the direction came from the guide. g == NULL is CRT_ERR_BAD_ARG: the unguided call exists. */
int crt_material_scatter_guided_n(CrtGuiding *g, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                                  size_t n, CrtScatterSample *d_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
