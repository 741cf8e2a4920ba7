/* libcrt_amd: volume renders — the one entry point that binds a volume aggregate (crt.h, CrtVolumes) to a wavefront
 * renderer (crt.h, CrtRenderer). A header of its own beside crt.h: crt.h's set of declarations is pinned as it stood
 * when the aggregate went behind the ABI (tests/test_volumes.py), and this entry point came after. Exported by the same
 * library; include it after, or instead of, crt.h. */
#ifndef CRT_RENDER_VOLUMES_H
#define CRT_RENDER_VOLUMES_H

#include "crt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Binds a volume aggregate to a renderer (the `volumes` of Renderer::render, tracer.rs:1167-1254), or detaches it
 * (v == NULL). The renderer keeps a reference of its own; the image is uploaded inside the call; the binding holds from
 * the next crt_render_samples on. A bound renderer runs one launch per stage whatever the batch size, with a volume
 * stage between extend and shade: per path segment Volumes::sample_interaction over (0.001, min(t_surface, t_medium)),
 * seeded off new_domain(v, K_VOLUME) of the vertex domain v (pattern ^ (index * 0x9e3779b9 + 0x7f4a7c15): the word
 * draw_rnd hashes), emission and weight folded into the path, a scatter turned into a phase vertex
 * (PhaseMix direction, volume_nee, roulette); a depth-exhausted segment and every shadow segment (seeded off
 * new_domain(v, K_NEE_SHADOW)) are attenuated by Volumes::transmittance. A walk that reaches
 * CRT_VOLUME_STEP_LIMIT is the all-zero event — weight 0, emitted 0, transmittance 0 — and raises no error. Where no
 * region is crossed the image and the counters are, bit for bit, those of the unbound renderer. DESIGN.md §2 has the
 * arithmetic. Waits for the renderer's batches in flight. CRT_ERR_BAD_ARG: r == NULL; CRT_ERR_NO_DEVICE: the upload failed;
 * CRT_ERR_UNSUPPORTED: an A/B build that regenerates camera paths in shade (CRT_REGEN_FIRST), which holds no volume stage. */
int crt_renderer_set_volumes(CrtRenderer *r, CrtVolumes *v);

#ifdef __cplusplus
}
#endif

#endif
