/* libcrt_amd: guided renders — the one entry point that binds a path guiding field (crt_guiding.h, CrtGuiding) to a
 * wavefront renderer (crt.h, CrtRenderer). A header of its own beside crt.h and crt_guiding.h: their sets of declarations
 * are pinned as they stood (tests/test_volumes.py, tests/test_guiding.py), and this entry point came after. Exported by
 * the same library; include it after, or instead of, the two. */
#ifndef CRT_RENDER_GUIDING_H
#define CRT_RENDER_GUIDING_H

#include "crt_guiding.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Binds a guiding field to a renderer, or detaches it (g == NULL): the batches that follow are the GUIDED PASS of
 * render_guided (tracer.rs:245-403) — render_pass(.., Some(&GuidingContext{field, training: false})). Nothing else of
 * render_guided is built: the renderer records no training sample, runs no pass schedule and blends nothing; whoever owns
 * the field trains it (crt_guiding_update) — a host integrator on the seam, or a test — and binds it here. The renderer
 * reads no crust:pathGuiding setting.
 *
 * At every surface vertex that has a previous vertex (tracer.rs:1386: not the camera vertex, not the vertex behind an
 * interior-medium scatter) where the field is trained (trained_at(p), field.rs:81-83): the bounce is
 * sample_bounce_direction (tracer.rs:777-826, the arithmetic of crt_material_scatter_guided_n) off the vertex domain, its
 * mixture pdf is what the next vertex's emission weight competes with, and the NEE weight's bounce pdf is
 * alpha * field.pdf(p, light_dir) + (1 - alpha) * brdf_pdf (tracer.rs:1432-1440). Every other vertex runs the unbound
 * renderer's arithmetic: with an untrained field, image and counters are, bit for bit, those of the unbound renderer.
 * DESIGN.md §2 has the guided-forward form.
 *
 * The renderer keeps a reference of its own: crt_guiding_free drops the caller's, and the field lives until the renderer
 * lets go of it. The image is uploaded inside the call. crt_guiding_update may rebuild the field between two
 * crt_render_samples calls: every crt_render_samples asks for the current image at its head (and uploads it then, after
 * waiting for the device) — crt_guiding.h's rule stands: no update while launches are in flight. A bound renderer runs one
 * launch per stage whatever the batch size, with the GUIDED shade instances; crt_renderer_pipeline reports | 1024 in
 * out[1]. Waits for the renderer's batches in flight.
 * CRT_ERR_BAD_ARG: r == NULL; CRT_ERR_NO_DEVICE: the upload failed; CRT_ERR_UNSUPPORTED, with the reason in
 * crt_last_error: a volume aggregate or a per-face texture aggregate is bound (crt_renderer_set_volumes and
 * crt_renderer_set_face_textures refuse a bound field likewise), or an A/B build that regenerates camera paths in shade
 * (CRT_REGEN_FIRST). crt_render_samples_stats refuses a renderer with a field bound (CRT_ERR_UNSUPPORTED). */
int crt_renderer_set_guiding(CrtRenderer *r, CrtGuiding *g);

#ifdef __cplusplus
}
#endif

#endif
