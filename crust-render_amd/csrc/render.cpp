// The wavefront path tracer's host side: Renderer (tracer.rs:137-148) — lanes, buffers, the bounce loop — and the
// renderer entry points of the C ABI, over the kernels of kernels/pathtrace.hip. What it knows of them is
// render_kernels.h: the launch argument types, kernel pointers resolved from a launch plan's keys (resolve_kernels), the
// single-form kernels (kStageKernels) and what the kernel headers know about the build (kKernelBuild). No device code.
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "render_kernels.h"
#include "face_textures_internal.h"
#include "guiding_internal.h"
#include "../../include/crt_render_guiding.h"

namespace crt {

using dev::DevMaterial;
using dev::DevMedium;
using dev::EnvSlot;
using dev::PixelRec;

struct Renderer {
  std::shared_ptr<Scene> scene;
  Params P{};
  std::vector<uint32_t> pixels;  // owned pixels (linear buffer index), tile order
  // One wavefront batch's buffers: path state (two buffers), hit records, shadow queue, staging film, queue counters.
  // LANES: a batch of n samples runs as up to kMaxLanes sub-batches of n / lanes consecutive samples, each with its own
  // buffers and counters on its own HIP stream, so the launches of one sub-batch overlap the other's — the ramp-up and
  // the drain of a launch (workgroups of its last round finishing one by one) are filled by the other lane's work, and a
  // traversal launch (latency and issue bound) runs beside a shade launch (the one that moves bytes). The film fold
  // stays on the caller's stream, lane after lane, so samples are summed in the same order as in one batch: bits unchanged.
  struct Lane {
    size_t cap_slots = 0;          // path slots (segment capacity x segments) the buffers are sized for
    char *blob = nullptr;
    size_t blob_bytes = 0;
    PathSoA S[2]{};
    HitSoA H{};
    ShadowSoA Q{};
    uint4 *fplane = nullptr;       // textured renders: the hit's (prim_id, u, v, 0) record, slot for slot beside H
    uint32_t *qseed = nullptr;     // volume renders of lit scenes: the K_NEE_SHADOW seed of every shadow-queue slot
    Counters *C = nullptr;
    float4 *staging = nullptr;
    hipStream_t stream = nullptr;  // lanes 1.. only (lane 0 runs on the caller's stream)
    hipEvent_t done = nullptr;
  };
  static constexpr int kMaxLanes = 4;
  Lane lanes[kMaxLanes];
  int n_lanes = 4;               // CRT_LANES; a batch is split only while every lane keeps lane_min_paths paths
  int last_lanes = 1;            // of the last batch (crt_renderer_lanes)
  size_t lane_min_paths = (size_t)96 << 20;
  hipEvent_t ev_start = nullptr;
  float4 *film = nullptr;
  CrtMaterial *d_materials = nullptr;
  DevMaterial *d_mat_derived = nullptr;  // one per record of d_materials (k_derive_materials)
  uint8_t *d_mat_class = nullptr;  // material_class() per record of d_materials
  uint16_t *d_mat_index = nullptr; // geom_id -> record, when the table is deduplicated (Params::mat_index)
  DevMedium *d_media = nullptr;  // [n_materials] by geom_id, then [n_materials] by compact id
  bool has_media = false;
  // adaptive stopping (variance_threshold > 0): per-pixel luminance statistics, sample counts and the active list
  PixelStats *d_pstats = nullptr;
  uint32_t *d_state = nullptr, *d_active = nullptr, *d_count = nullptr;
  uint32_t n_act = 0, min_spp = 2;
  float variance_threshold = 0.0f;
  // Which kernel instances run a batch: plan_launches (launch_plan.h) decides from `in` — the image's engine choice
  // (select_engine), the tables, the A/B knobs and this build's switches, filled at creation; the batch's path count and
  // whether it is the stats build, set per batch — and render_lane launches what the instance table below holds for the
  // plan's keys. last_plan: what the LAST batch ran (crt_renderer_pipeline); until the first, the scene's preference.
  PlanInputs in;
  LaunchPlan last_plan;
  // The bound volume aggregate (crt_renderer_set_volumes): a reference of the renderer's own, and its device image as the
  // kernels take it. nullptr: none — every batch then runs what it ran before volumes existed.
  CrtVolumes *volumes = nullptr;
  VolArgs vol{nullptr, nullptr, 0};
  // The bound per-face texture aggregate (crt_renderer_set_face_textures): a reference of the renderer's own, and its device
  // tables as the kernels take them. nullptr: none — every batch then runs what it ran before textures existed.
  CrtFaceTextures *faces = nullptr;
  dev::FaceView face_view{};
  // The bound guiding field (crt_renderer_set_guiding): a reference of the renderer's own, and the view of its device image
  // as the GUIDED shade instances take it — asked of guiding_device at the head of every render call, since
  // crt_guiding_update may have rebuilt the image in between. nullptr: none — every batch runs what it ran before.
  CrtGuiding *guiding = nullptr;
  dev::GuideView guide_view{};
  uint32_t n_materials_given = 0;  // the caller's table at creation, before any deduplication: what material bindings index
  // What the root cull can save grows with the share of the frame that shows background; what it costs does not:
  // generate's slab tests and compaction, plane d beside the compact form. So the renderer looks first: the root step of
  // the pixel-centre rays of a 32 x 18 grid over the frame, through the lens centre, on the host (at creation), and
  // plan_launches culls only where at least kRootCullMinShare of them miss every child of the root.
  void estimate_root_miss_share() {
    in.root_miss_share = 0.0f;
    if (!scene || scene->bvh.wide.empty()) return;
    const WideNode &nd = scene->bvh.wide[0];  // the committed tree's root (bvh.rs:442-447): the image's root node, child words apart
    uint32_t child[4];
    for (int l = 0; l < 4; l++) child[l] = (nd.flags & (1u << l)) ? 0u : CRT_INVALID_ID;
    const CrtCamera &c = P.camera;
    constexpr int GW = 32, GH = 18;
    int missed = 0;
    for (int j = 0; j < GH; j++)
      for (int i = 0; i < GW; i++) {
        const float sx = ((float)i + 0.5f) / (float)GW, sy = ((float)j + 0.5f) / (float)GH;
        float d[3];
        for (int a = 0; a < 3; a++) d[a] = c.lower_left[a] + c.horizontal[a] * sx + c.vertical[a] * sy - c.origin[a];
        if (!node_touched(nd.bmin, nd.bmax, child, c.origin[0], c.origin[1], c.origin[2], d[0], d[1], d[2], 0.001f, INFINITY)) missed++;
      }
    in.root_miss_share = (float)missed / (float)(GW * GH);
  }
  size_t max_batch_slots = 0;     // CRT_MAX_BATCH_SLOTS (tests): ensure_buffers fails above this many slots; 0 = no limit
  int cus = 256, fused_mult = 3, stage_mult = 8, mult_forced = 0;
  CrtLight *d_lights = nullptr;
  std::vector<std::shared_ptr<void>> environments;  // what the mapped domes of the light list name (Params::envs is set iff any)
  uint32_t *d_pixels = nullptr;
  // One PixelRec per owned-pixel slot (kernels/camera_pixel.hip.h), filled once at creation where a plan of this renderer
  // can read it; nullptr: none was built (no such plan, CRT_PIXEL_TABLE=0, or no memory — the computed form then runs).
  PixelRec *d_pixel_table = nullptr;
  int grid = 768;         // of the last batch; the film kernels use it too
  hipStream_t last_stream = nullptr;
  bool profile = false;
  struct Ev { hipEvent_t a, b; int cls; };
  std::vector<Ev> events;
  double prof_ms[4] = {0, 0, 0, 0};
  uint64_t prof_launches[4] = {0, 0, 0, 0};

  ~Renderer() {
    drain_events();
    for (Lane &B : lanes) {
      if (B.stream) (void)hipStreamSynchronize(B.stream);  // nothing of a lane may be in flight when its buffers go
      if (B.blob) (void)hipFree(B.blob);
      if (B.C) (void)hipFree(B.C);
      if (B.stream) (void)hipStreamDestroy(B.stream);
      if (B.done) (void)hipEventDestroy(B.done);
    }
    if (ev_start) (void)hipEventDestroy(ev_start);
    guiding_release(guiding);  // behind the synchronised lanes, like the two below
    face_textures_release(faces);
    volumes_release(volumes);  // behind the synchronised lanes; the caller's stream is the caller's to drain (as for the scene)
    if (film) (void)hipFree(film);
    if (d_materials) (void)hipFree(d_materials);
    if (d_mat_derived) (void)hipFree(d_mat_derived);
    if (d_mat_class) (void)hipFree(d_mat_class);
    if (d_mat_index) (void)hipFree(d_mat_index);
    if (d_media) (void)hipFree(d_media);
    if (d_pstats) (void)hipFree(d_pstats);
    if (d_state) (void)hipFree(d_state);
    if (d_active) (void)hipFree(d_active);
    if (d_count) (void)hipFree(d_count);
    if (d_lights) (void)hipFree(d_lights);
    if (d_pixels) (void)hipFree(d_pixels);
    if (d_pixel_table) (void)hipFree(d_pixel_table);
  }

  void drain_events() {
    for (Ev &e : events) {
      float ms = 0.0f;
      if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
        prof_ms[e.cls] += ms;
        prof_launches[e.cls]++;
      }
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    events.clear();
  }

  // Workgroups (= queue segments) of a batch of `total` paths. Fused: 3 per CU, what stays resident (LDS of the
  // traversal engine), so a wave's ray pool drains once per launch; per-stage: 8 — two rounds of the four resident
  // workgroups. Either is doubled while a segment would hold more than 192 Ki paths: past that, shorter segments balance
  // better than longer ones drain (per-stage, cornellbox 1080p, Mray/s: 128 spp x8 8179, x12 8011, x16 7490; 256 spp x8
  // 8420, x16 8630, x32 8655 — fused, 531 M paths: MedCity x3 1985, x6 1997, x12 2028, x24 2041; openpbr_showcase 12077,
  // 12142, 12179, 12067; 133 M paths: openpbr_showcase x3 11579, x6 11426, x12 11152). Only power-of-two multiples deal
  // the camera samples evenly (per-stage x6 7066, x10 7397, x12 8011, x20 8318).
  int batch_grid(size_t total, bool fused_pipeline) const {
    int mult = fused_pipeline ? fused_mult : stage_mult;
    if (!mult_forced)
      while (mult < 64 && total / ((size_t)cus * mult) > ((size_t)192 << 10)) mult *= 2;
    const int g = cus * mult;
    return g > kMaxGrid ? kMaxGrid : g;
  }

  int ensure_buffers(Lane &B, size_t slots) {  // slots = segment capacity x segments of the batch about to run
    size_t &cap_slots = B.cap_slots, &blob_bytes = B.blob_bytes;
    char *&blob = B.blob;
    PathSoA (&S)[2] = B.S;
    HitSoA &H = B.H;
    ShadowSoA &Q = B.Q;
    float4 *&staging = B.staging;
    // grow only — except that a lane of a multi-lane batch gives back a buffer sized for a whole batch (a single-lane
    // call before it, e.g. the stats pass): four lanes next to one whole-batch buffer would not fit the HBM
    if (slots <= cap_slots && blob && !(last_lanes > 1 && cap_slots > slots + slots / 2)) return CRT_OK;
    if (blob) { (void)hipFree(blob); blob = nullptr; }
    const size_t total = slots, cap = slots;  // shadow queue and staging film: one slot per path
    const size_t bcap = cap * kBins;      // path and hit planes: one sub-segment per (workgroup, direction bin)
    if (total == 0 || bcap >= (size_t)0x7fffffff) return CRT_ERR_BAD_ARG;
    const size_t p16 = (cap * 16 + 255) & ~size_t(255);
    const size_t b16 = (bcap * 16 + 255) & ~size_t(255), b4 = (bcap * 4 + 255) & ~size_t(255);
    const bool lit = P.n_lights > 0, motion = P.has_motion != 0;
    const size_t f16 = faces ? b16 : 0;  // the hit's face record plane (set_face_textures frees the blobs)
    const size_t p4 = (lit && volumes) ? ((cap * 4 + 255) & ~size_t(255)) : 0;  // the shadow queue's seed plane (set_volumes frees the blobs)
    // 2 x (a b c d [e] [16 B] + [time 4 B]) + hit (16 + 4) + shadow 3 x 16 [+ 4] + staging 16
    blob_bytes = 2 * ((lit ? 5 : 4) * b16 + (motion ? b4 : 0)) + (b16 + b4) + f16 + (lit ? 3 * p16 : 0) + p4 + p16;
    // CRT_MAX_BATCH_SLOTS (tests): a batch of more slots asks for more memory than any device has, so the allocation
    // fails the way it does on a part with too little free HBM (bench.py halves the batch then).
    const size_t want_bytes = (max_batch_slots && slots > max_batch_slots) ? ((size_t)1 << 46) : blob_bytes;
    if (!CRT_HIP_OK(hipMalloc(&blob, want_bytes))) {
      // hipGetLastError returns the last ERROR, not the last call's status: left in place, the out-of-memory would be
      // reported by the next successful batch's launch check (a retry with a smaller batch would fail for no reason)
      (void)hipGetLastError();
      blob = nullptr; blob_bytes = 0; cap_slots = 0;
      return CRT_ERR_NO_DEVICE;
    }
    char *cur_p = blob;
    auto take = [&](size_t bytes) { char *r = cur_p; cur_p += bytes; return r; };
    for (int b = 0; b < 2; b++) {
      S[b].a = (float4 *)take(b16); S[b].b = (float4 *)take(b16); S[b].c = (float4 *)take(b16);
      S[b].d = (uint4 *)take(b16);
      S[b].e = lit ? (float4 *)take(b16) : nullptr;
      S[b].time = motion ? (float *)take(b4) : nullptr;
    }
    H.h = (float4 *)take(b16); H.geom = (uint32_t *)take(b4);
    B.fplane = f16 ? (uint4 *)take(f16) : nullptr;
    if (lit) { Q.a = (float4 *)take(p16); Q.b = (float4 *)take(p16); Q.c = (float4 *)take(p16); }
    B.qseed = p4 ? (uint32_t *)take(p4) : nullptr;
    staging = (float4 *)take(p16);
    cap_slots = cap;
    return CRT_OK;
  }

  template <class F>
  void timed(int cls, hipStream_t st, F &&launch) {
    if (!profile) { launch(); return; }
    Ev e; e.cls = cls;
    (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b);
    (void)hipEventRecord(e.a, st);
    launch();
    (void)hipEventRecord(e.b, st);
    events.push_back(e);
  }

  int render(uint32_t sample_begin, uint32_t n_samples, hipStream_t st, CrtTravStats *d_tstats) {
    if (n_samples == 0) return CRT_OK;
    if (n_samples > 0xffffu) return CRT_ERR_BAD_ARG;
    (void)hipGetLastError();  // launches below are checked against a clean slate, not against an earlier call's error
    // the field's current image: crt_guiding_update may have rebuilt it since the last call (the upload waits for the device)
    if (guiding)
      if (const int rc = guiding_device(guiding, guide_view)) return rc;
    last_stream = st;
    // how many lanes: one for the stats build and adaptive stopping (the active list changes between batches) and for
    // batches too small to fill the chip twice over
    int L = n_lanes;
    const size_t total = (size_t)P.n_pix * n_samples;
    if (d_tstats || variance_threshold > 0.0f) L = 1;
    while (L > 1 && (total / L < lane_min_paths || n_samples < (uint32_t)L)) L--;
    last_lanes = L < 1 ? 1 : L;
    // lanes this batch does not use give their buffers back first: a whole batch in lane 0 next to the quarter batches of
    // an earlier call's other lanes would not fit (the stats pass behind a four-lane batch of a lit scene: 259 + 195 GB)
    for (int l = L < 1 ? 1 : L; l < kMaxLanes; l++) {
      Lane &B = lanes[l];
      if (!B.blob) continue;
      if (B.stream) (void)hipStreamSynchronize(B.stream);
      (void)hipFree(B.blob);
      B.blob = nullptr; B.cap_slots = 0; B.blob_bytes = 0;
    }
    if (L <= 1) return render_lane(lanes[0], sample_begin, n_samples, st, d_tstats, true);
    if (!ev_start && !CRT_HIP_OK(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming))) return CRT_ERR_NO_DEVICE;
    for (int l = 1; l < L; l++) {
      Lane &B = lanes[l];
      if (!B.stream && !CRT_HIP_OK(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking))) return CRT_ERR_NO_DEVICE;
      if (!B.done && !CRT_HIP_OK(hipEventCreateWithFlags(&B.done, hipEventDisableTiming))) return CRT_ERR_NO_DEVICE;
    }
    uint32_t begin[kMaxLanes], count[kMaxLanes];
    for (int l = 0; l < L; l++) {
      count[l] = n_samples / L + ((uint32_t)l < n_samples % L ? 1u : 0u);
      begin[l] = l == 0 ? sample_begin : begin[l - 1] + count[l - 1];
    }
    // every lane's buffers BEFORE any launch: an allocation that fails then fails with nothing of this batch in flight
    for (int l = 0; l < L; l++) {
      Params scratch = P;
      const int rc = plan_lane(lanes[l], scratch, count[l], false);
      if (rc != CRT_OK) return rc;
    }
    // every lane starts behind what the caller's stream has queued (the previous batch's film fold reads the staging
    // films this batch overwrites); lane 0 IS the caller's stream
    if (!CRT_HIP_OK(hipEventRecord(ev_start, st))) return CRT_ERR_NO_DEVICE;
    // a failure from here on leaves launches in flight on the lanes' own (non-blocking) streams, which nothing the caller
    // does afterwards waits for (crt_render_stats, crt_film_clear, a retry sync only the caller's stream): drain them
    auto fail = [&](int rc) {
      for (int l = 1; l < L; l++)
        if (lanes[l].stream) (void)hipStreamSynchronize(lanes[l].stream);
      (void)hipStreamSynchronize(st);
      return rc;
    };
    // the lanes on their own streams first, lane 0 on the caller's last: its launches then queue behind nothing of ours
    for (int l = L - 1; l >= 0; l--) {
      hipStream_t ls = l == 0 ? st : lanes[l].stream;
      if (l > 0 && !CRT_HIP_OK(hipStreamWaitEvent(ls, ev_start, 0))) return fail(CRT_ERR_NO_DEVICE);
      const int rc = render_lane(lanes[l], begin[l], count[l], ls, nullptr, false);
      if (rc != CRT_OK) return fail(rc);
      if (l > 0 && !CRT_HIP_OK(hipEventRecord(lanes[l].done, ls))) return fail(CRT_ERR_NO_DEVICE);
    }
    // the film fold: lane after lane on the caller's stream = sample order
    for (int l = 0; l < L; l++) {
      if (l > 0 && !CRT_HIP_OK(hipStreamWaitEvent(st, lanes[l].done, 0))) return fail(CRT_ERR_NO_DEVICE);
      timed(3, st, [&] { hipLaunchKernelGGL(kStageKernels.resolve, dim3(grid), dim3(kBlock), 0, st, lanes[l].staging, P.n_pix, count[l], film); });
    }
    return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : fail(CRT_ERR_NO_DEVICE);
  }

  // The launch plan of one lane's batch of n_samples (launch_plan.h, plan_launches), its grid and segment size, and its
  // buffers (they grow when a batch needs more slots than any before). Sets last_plan / grid for the launches that
  // follow, and p.seg_cap, p.cam_compact, p.root_cull.
  // from P at every plan, so that nothing set after creation leaves the plan stale; the engine choice, mats_kind and
  // the root's miss share are derived at creation from what no entry point changes (the image, the table, the camera)
  void plan_inputs_from_params() {
    in.scene = P.scene;
    in.n_lights = P.n_lights; in.has_inf_lights = P.has_inf_lights != 0; in.has_env = P.envs != nullptr; in.strategy = P.strategy;
    in.has_motion = P.has_motion != 0; in.lens = P.camera.lens_radius > 0.0f;
    in.mat_index = P.mat_index != nullptr; in.partition = P.partition; in.n_materials = P.n_materials; in.max_depth = P.max_depth;
    in.class_stats = P.class_stats;
    in.volumes = volumes != nullptr;
    in.faces = faces != nullptr;
    in.guided = guiding != nullptr;
  }
  // The per-pixel camera table (kernels/camera_pixel.hip.h), at creation: built where the plan of a large batch of this
  // renderer names it — asked of plan_launches itself, so the rule stays in one place. No memory for it (32 bytes per
  // owned pixel) or a frame wider than the records' float coordinates hold: no table, and every plan runs the computed form.
  void build_pixel_table() {
    in.pixel_table_ready = false;
    if (in.pixel_table_knob == 0 || P.width > kPixelTableMaxExtent || P.height > kPixelTableMaxExtent) return;
    plan_inputs_from_params();
    PlanInputs q = in;
    q.total = ~(size_t)0 >> 1; q.stats = false; q.partial_active = false; q.pixel_table_ready = true;
    LaunchPlan trial;
    if (plan_launches(q, trial) != CRT_OK || !trial.pixel_table) return;
    if (hipMalloc(&d_pixel_table, (size_t)P.n_pix * kKernelBuild.sizeof_pixel_rec) != hipSuccess) {
      (void)hipGetLastError();  // not an error: the computed form
      d_pixel_table = nullptr;
      return;
    }
    hipLaunchKernelGGL(kStageKernels.fill_pixel_table, dim3((P.n_pix + 255) / 256), dim3(256), 0, nullptr, P.pixel_index, P.n_pix, P.width,
                       P.frame, d_pixel_table);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {  // filled before any lane's stream reads it
      (void)hipFree(d_pixel_table);
      d_pixel_table = nullptr;
      return;
    }
    in.pixel_table_ready = true;
  }

  int plan_lane(Lane &B, Params &p, uint32_t n_samples, bool stats) {
    const size_t total = (size_t)p.n_act * n_samples;
    in.total = total;
    in.stats = stats;
    plan_inputs_from_params();
    in.partial_active = p.active != nullptr;
    if (in.volumes && stats) {
      set_error_text("render refused: the stats build does not run volume renders");
      return CRT_ERR_UNSUPPORTED;
    }
    if (in.faces && (stats || in.volumes)) {
      set_error_text("render refused: textured renders run neither the stats build nor beside volumes");
      return CRT_ERR_UNSUPPORTED;
    }
    if (in.guided && (stats || in.volumes || in.faces)) {
      set_error_text("render refused: guided renders run neither the stats build nor beside volumes or textures");
      return CRT_ERR_UNSUPPORTED;
    }
    if (plan_launches(in, last_plan) != CRT_OK) {
      set_error_text("render refused: the selected kernels (wide %d, cold %d / %d) cannot run this image (direct words %u, cold %u)",
                     (int)last_plan.wide, last_plan.ext_cold, last_plan.path_cold, P.scene.direct_leaves, P.scene.cold);
      return CRT_ERR_UNSUPPORTED;
    }
    grid = batch_grid(total, last_plan.fused);
    p.seg_cap = (uint32_t)(((total + (size_t)grid * kBlock - 1) / ((size_t)grid * kBlock)) * kBlock);
    p.cam_compact = last_plan.cam_compact;
    p.root_cull = last_plan.root_cull ? 1u : 0u;
    if (const int rc = ensure_buffers(B, (size_t)p.seg_cap * grid)) return rc;  // >= total: the staging film's (sample, active pixel) slots too
    // the slim path state keeps a flag in bit 31 of the pixel word: pixel < n_act <= slots < 2^31 (ensure_buffers)
    if (last_plan.slim_state && p.n_act > 0x7fffffffu) {
      set_error_text("render refused: %u active pixels do not fit the slim path state's 31 bits", p.n_act);
      return CRT_ERR_BAD_ARG;
    }
    return CRT_OK;
  }

  int render_lane(Lane &B, uint32_t sample_begin, uint32_t n_samples, hipStream_t st, CrtTravStats *d_tstats, bool fold_here) {
    PathSoA (&S)[2] = B.S;
    HitSoA &H = B.H;
    ShadowSoA &Q = B.Q;
    Counters *C = B.C;
    const bool adaptive = variance_threshold > 0.0f;
    if (adaptive && n_act == 0) return CRT_OK;  // every pixel has stopped
    Params p = P;
    p.sample_begin = sample_begin;
    p.n_act = adaptive ? n_act : P.n_pix;
    p.active = (adaptive && n_act < P.n_pix) ? d_active : nullptr;
    if (const int rc = plan_lane(B, p, n_samples, d_tstats != nullptr)) return rc;
    const LaunchPlan plan = last_plan;
    if (plan.volumes != (volumes != nullptr)) return CRT_ERR_UNSUPPORTED;
    if (plan.faces != (faces != nullptr) || (plan.faces && !B.fplane)) return CRT_ERR_UNSUPPORTED;
    if (plan.guided != (guiding != nullptr)) return CRT_ERR_UNSUPPORTED;
    BatchKernels k;
    if (const int rc = resolve_kernels(plan, k)) return rc;
    float4 *staging = B.staging;
    // the film fold: plain sum, or with the luminance statistics and the stopping rule, then the new active list
    auto fold = [&]() -> int {
      if (!fold_here) return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE;  // the caller folds the lanes in order
      if (!adaptive) {
        timed(3, st, [&] { hipLaunchKernelGGL(kStageKernels.resolve, dim3(grid), dim3(kBlock), 0, st, staging, P.n_pix, n_samples, film); });
        return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE;
      }
      timed(3, st, [&] {
        hipLaunchKernelGGL(kStageKernels.resolve_adaptive, dim3(grid), dim3(kBlock), 0, st, staging, p.active, p.n_act, n_samples, film,
                           d_pstats, d_state, min_spp, variance_threshold);
        (void)hipMemsetAsync(d_count, 0, 4, st);
        hipLaunchKernelGGL(kStageKernels.compact_active, dim3(grid), dim3(kBlock), 0, st, d_state, P.n_pix, d_active, d_count);
      });
      uint32_t h = 0;  // the next batch's size is a launch parameter: one 4-byte read-back per batch
      if (!CRT_HIP_OK(hipMemcpyAsync(&h, d_count, 4, hipMemcpyDeviceToHost, st)) || !CRT_HIP_OK(hipStreamSynchronize(st)))
        return CRT_ERR_NO_DEVICE;
      n_act = h;
      return CRT_OK;
    };
    if (plan.fused) {  // one launch for the whole path loop (class 0 of the profile), then the film fold
      timed(0, st, [&] { hipLaunchKernelGGL(k.path, dim3(grid), dim3(kBlock), 0, st, p, S[0], S[1], H, Q, C, staging, sample_begin, n_samples, 0u, 0); });
      return fold();
    }
    // generate — or, where the plan says so, k_camera: generate, cull and the camera rays' traversal in one launch, whose
    // first extend below only picks up the rays it deferred
    // — or k_camera_vertex: the same with the first vertex shaded behind the trace; its survivors are in S[1] already, and
    // the first extend and the first shade (append mode, bit 1 of `first`) see only the rays it deferred, which lie in S[0]
    // in the compact form with plane d whatever the cull says
    const PixelRec *pixel_table = plan.pixel_table ? d_pixel_table : nullptr;  // plan.pixel_table: the renderer holds one
    if (plan.pixel_table && !pixel_table) return CRT_ERR_UNSUPPORTED;
    Params p0 = p;  // the launches of bounce 0 behind k_camera_vertex
    if (plan.camera_vertex) {
      p0.cam_compact = 2;
      const uint32_t nx = 1;
      const int slim_out = (k.shade_slim && nx <= P.max_depth && nx < plan.tail_at && (int)nx < plan.noclassify_from) ? 1 : 0;
      timed(3, st, [&] { hipLaunchKernelGGL(k.camera_vertex, dim3(grid), dim3(kBlock), 0, st, p, S[0], S[1], C, sample_begin, n_samples, staging, plan.camera_mode, slim_out, pixel_table); });
    } else if (plan.camera_trace)
      timed(3, st, [&] { hipLaunchKernelGGL(k.camera, dim3(grid), dim3(kBlock), 0, st, p, S[0], reinterpret_cast<uint32_t *>(S[1].a), H, C, sample_begin, n_samples, staging, plan.camera_mode, pixel_table); });
    else
      timed(3, st, [&] { hipLaunchKernelGGL(kStageKernels.generate, dim3(grid), dim3(kBlock), 0, st, p, S[0], C, sample_begin, n_samples, staging); });
    int cur = 0;
    for (uint32_t it = 0; it <= P.max_depth; it++) {
      if (it >= plan.tail_at) {  // the tail: what is left of the batch in one launch of the path-loop kernel
        timed(3, st, [&] { hipLaunchKernelGGL(k.path, dim3(grid), dim3(kBlock), 0, st, p, S[0], S[1], H, Q, C, staging, sample_begin, n_samples, it, cur); });
        break;
      }
      const int first = it == 0 ? 1 : 0;
      if (first && plan.camera_vertex)
        timed(0, st, [&] { hipLaunchKernelGGL(k.extend, dim3(grid), dim3(kBlock), 0, st, p0, S[cur], H, C, cur, first, d_tstats); });
      else if (first && plan.camera_trace)
        timed(0, st, [&] { hipLaunchKernelGGL(k.extend_deferred, dim3(grid), dim3(kBlock), 0, st, p, S[cur], H, C, cur, first, d_tstats, reinterpret_cast<const uint32_t *>(S[1 - cur].a)); });
      else if (plan.faces)  // the FACES instance: the hit's (prim_id, u, v) kept beside the record
        timed(0, st, [&] { hipLaunchKernelGGL(k.extend_faces, dim3(grid), dim3(kBlock), 0, st, p, S[cur], H, C, cur, first, d_tstats, B.fplane); });
      else
        timed(0, st, [&] { hipLaunchKernelGGL(k.extend, dim3(grid), dim3(kBlock), 0, st, p, S[cur], H, C, cur, first, d_tstats); });
      if (plan.faces) {  // the FACES shade instance (MatFace)
        timed(1, st, [&] { hipLaunchKernelGGL(k.shade_faces, dim3(grid), dim3(kBlock), 0, st, p, S[cur], S[1 - cur], H, Q, C, cur, staging, first | ((int)it >= plan.noclassify_from ? 2 : 0), face_view, (const uint4 *)B.fplane); });
      } else if (plan.guided) {  // the GUIDED shade instance (the field's view by value)
        timed(1, st, [&] { hipLaunchKernelGGL(k.shade_guided, dim3(grid), dim3(kBlock), 0, st, p, S[cur], S[1 - cur], H, Q, C, cur, staging, first | ((int)it >= plan.noclassify_from ? 2 : 0), guide_view); });
      } else if (plan.volumes) {  // the walk, then the VOL shade instance (plane c is k_volume's to write: never `first`), then the shadow segments' walk
        timed(3, st, [&] { hipLaunchKernelGGL(kStageKernels.volume, dim3(grid), dim3(kBlock), 0, st, p, S[cur], H, C, cur, first, vol); });
        timed(1, st, [&] { hipLaunchKernelGGL(k.shade_vol, dim3(grid), dim3(kBlock), 0, st, p, S[cur], S[1 - cur], H, Q, C, cur, staging, (int)it >= plan.noclassify_from ? 2 : 0, B.qseed); });
        if (!plan.shadow_volume_key.none())
          timed(3, st, [&] { hipLaunchKernelGGL(kStageKernels.shadow_volume, dim3(grid), dim3(kBlock), 0, st, p, Q, (const uint32_t *)B.qseed, C, vol); });
      } else if (k.shade_pipe && (int)it < plan.noclassify_from) {  // the pipelined instance (shade_segment_pipe)
        // Slim state (plan.slim_state): the launch writes the full form where the next consumer of its output is not
        // this kernel again — the tail, the plain k_shade from noclassify_from, or nothing past the depth limit.
        const uint32_t nx = it + 1;
        const int out_full = (nx <= P.max_depth && nx < plan.tail_at && (int)nx < plan.noclassify_from) ? 0 : 1;
        const ShadePipeFn fn = k.shade_slim ? k.shade_slim : k.shade_pipe;
        if (first && plan.camera_vertex)
          timed(1, st, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), 0, st, p0, S[cur], S[1 - cur], H, C, cur, staging, first | 2, it, out_full); });
        else
          timed(1, st, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), 0, st, p, S[cur], S[1 - cur], H, C, cur, staging, first, it, out_full); });
      } else
        timed(1, st, [&] { hipLaunchKernelGGL(k.shade, dim3(grid), dim3(kBlock), 0, st, p, S[cur], S[1 - cur], H, Q, C, cur, staging, first | ((int)it >= plan.noclassify_from ? 2 : 0)); });
      if (k.shadow)
        timed(2, st, [&] { hipLaunchKernelGGL(k.shadow, dim3(grid), dim3(kBlock), 0, st, p, S[1 - cur], Q, C, staging, d_tstats ? d_tstats + 1 : nullptr); });
      cur = 1 - cur;
    }
    return fold();
  }
};

}  // namespace crt

struct CrtRenderer { crt::Renderer r; };

using namespace crt;

extern "C" {

void crt_camera_new(CrtCamera *c, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov_deg,
                    float aspect, float aperture, float focus_dist) {  // camera.rs:27-63 (host-side setup)
  if (!c) return;
  auto sub = [](const float a[3], const float b[3], float o[3]) { for (int i = 0; i < 3; i++) o[i] = a[i] - b[i]; };
  auto nrm = [](float a[3]) {
    const float l = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    for (int i = 0; i < 3; i++) a[i] = a[i] / l;
  };
  auto crs = [](const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - b[1] * a[2]; o[1] = a[2] * b[0] - b[2] * a[0]; o[2] = a[0] * b[1] - b[0] * a[1];
  };
  const float theta = vfov_deg * 3.14159265358979323846f / 180.0f;
  const float h = tanf(theta / 2.0f);
  const float viewport_height = 2.0f * h;
  const float viewport_width = aspect * viewport_height;
  float w[3], u[3], v[3];
  sub(lookfrom, lookat, w); nrm(w);
  crs(vup, w, u); nrm(u);
  crs(w, u, v);
  for (int i = 0; i < 3; i++) {
    c->origin[i] = lookfrom[i];
    c->horizontal[i] = u[i] * (focus_dist * viewport_width);
    c->vertical[i] = v[i] * (focus_dist * viewport_height);
    c->lower_left[i] = ((lookfrom[i] - c->horizontal[i] / 2.0f) - c->vertical[i] / 2.0f) - w[i] * focus_dist;
    c->u[i] = u[i];
    c->v[i] = v[i];
  }
  c->lens_radius = aperture / 2.0f;
}

// The body of crt_renderer_new; it may throw (std containers of the pixel list, the material table's deduplication): the
// entry point below catches, `hold` frees what was built.
static CrtRenderer *renderer_new(CrtScene *scene, const CrtMaterial *materials, size_t n_materials, const CrtLight *lights,
                                 size_t n_lights, const CrtCamera *camera, const CrtRenderSettings *settings,
                                 uint32_t tile_rank, uint32_t tile_world) {
  if (!scene || !camera || !settings || (n_materials && !materials) || (n_lights && !lights)) return nullptr;
  if (tile_world == 0 || tile_rank >= tile_world) return nullptr;
  if (!(settings->variance_threshold >= 0.0f)) return nullptr;
  if (n_materials < scene->p->n_geoms) return nullptr;        // one material per geom_id (rt_world.rs:111-122)
  if (settings->max_depth > 0xffffu) return nullptr;
  if (scene->p->ensure_device() != CRT_OK) return nullptr;
  CrtRenderer *R = new (std::nothrow) CrtRenderer();
  if (!R) return nullptr;
  struct Hold { CrtRenderer *p; ~Hold() { delete p; } } hold{R};  // every way out but the last frees the renderer
  const Knobs knobs = read_knobs();
  Renderer &r = R->r;
  r.scene = scene->p;
  Params &P = r.P;
  P.scene = scene->p->dev->view;
  P.n_lights = (uint32_t)n_lights;
  P.n_materials = (uint32_t)n_materials;
  r.n_materials_given = (uint32_t)n_materials;
  P.has_inf_lights = 0;
  for (size_t k = 0; k < n_lights; k++) {
    if (lights[k].kind > CRT_LIGHT_DOME_MAP) { set_error_text("crt_renderer_new: light %zu has the unknown kind %u", k, lights[k].kind); return nullptr; }
    if (lights[k].kind >= CRT_LIGHT_DISTANT) P.has_inf_lights = 1;
    if (lights[k].kind == CRT_LIGHT_DOME_MAP) {  // retained like the scene; an id that names no live environment is refused
      uint32_t id;
      std::memcpy(&id, &lights[k].center[0], 4);
      std::shared_ptr<void> env = env_retain(id);
      if (!env) { set_error_text("crt_renderer_new: light %zu names environment id 0x%x, which is not live", k, id); return nullptr; }
      r.environments.push_back(std::move(env));
    }
  }
  P.envs = nullptr;
  if (!r.environments.empty()) {
    const void *table = nullptr;
    if (env_table_for_launch(&table) != CRT_OK || !table) return nullptr;
    P.envs = static_cast<const EnvSlot *>(table);
  }
  P.camera = *camera;
  P.width = settings->width; P.height = settings->height; P.max_depth = settings->max_depth;
  P.frame = settings->frame; P.strategy = settings->strategy; P.filter_kind = settings->filter_kind;
  P.filter_radius = settings->filter_radius;
  P.has_motion = scene->p->has_motion ? 1u : 0u;
  // Pixel-tile shard: 16x16 tiles (tracer.rs:424, :1671-1686) dealt round-robin over the ranks.
  r.pixels.resize(crt_shard_pixels(P.width, P.height, tile_rank, tile_world, nullptr));
  crt_shard_pixels(P.width, P.height, tile_rank, tile_world, r.pixels.data());
  P.n_pix = (uint32_t)r.pixels.size();
  P.n_act = P.n_pix; P.active = nullptr;
  r.variance_threshold = settings->variance_threshold;
  r.min_spp = settings->min_spp > 2 ? settings->min_spp : 2;  // tracer.rs:526
  r.n_act = P.n_pix;
  bool ok = P.n_pix > 0;
  if (ok && r.variance_threshold > 0.0f) {
    ok = CRT_HIP_OK(hipMalloc(&r.d_pstats, (size_t)P.n_pix * sizeof(PixelStats))) &&
         CRT_HIP_OK(hipMemset(r.d_pstats, 0, (size_t)P.n_pix * sizeof(PixelStats))) &&
         CRT_HIP_OK(hipMalloc(&r.d_state, (size_t)P.n_pix * 4)) && CRT_HIP_OK(hipMemset(r.d_state, 0, (size_t)P.n_pix * 4)) &&
         CRT_HIP_OK(hipMalloc(&r.d_active, (size_t)P.n_pix * 4)) && CRT_HIP_OK(hipMalloc(&r.d_count, 4));
  }
  for (Renderer::Lane &B : r.lanes)
    ok = ok && CRT_HIP_OK(hipMalloc(&B.C, sizeof(Counters))) && CRT_HIP_OK(hipMemset(B.C, 0, sizeof(Counters)));
  ok = ok && CRT_HIP_OK(hipMalloc(&r.film, (size_t)P.n_pix * 16)) && CRT_HIP_OK(hipMemset(r.film, 0, (size_t)P.n_pix * 16));
  ok = ok && CRT_HIP_OK(hipMalloc(&r.d_pixels, (size_t)P.n_pix * 4)) &&
       CRT_HIP_OK(hipMemcpy(r.d_pixels, r.pixels.data(), (size_t)P.n_pix * 4, hipMemcpyHostToDevice));
  // The material table: one record per geometry id, or — when that table would not fit shade's LDS arena and holds
  // repeats — the distinct records and a 2-byte index per geometry id (Params::mat_index). Everything below that is
  // "per material" (class byte, interior medium) is then per DISTINCT material. CRT_MAT_DEDUP=0: never (A/B, tests).
  std::vector<CrtMaterial> unique_mats;
  std::vector<uint16_t> mat_index;
  {
    bool dedup = kKernelBuild.mat_index && n_materials > (size_t)kKernelBuild.mat_lds_max;
    dedup = dedup && knobs.mat_dedup != 0;  // CRT_MAT_DEDUP=0
    if (dedup) {
      auto bytes_of = [](const CrtMaterial &m) { return std::string(reinterpret_cast<const char *>(&m), sizeof(CrtMaterial)); };
      std::unordered_map<std::string, uint32_t> seen;
      mat_index.resize(n_materials);
      for (size_t k = 0; k < n_materials && dedup; k++) {
        auto it = seen.emplace(bytes_of(materials[k]), (uint32_t)unique_mats.size());
        if (it.second) unique_mats.push_back(materials[k]);
        if (unique_mats.size() > 0xffffu) dedup = false;  // a 2-byte index
        mat_index[k] = (uint16_t)it.first->second;
      }
      if (!dedup || unique_mats.size() == n_materials) { unique_mats.clear(); mat_index.clear(); }
    }
  }
  if (!unique_mats.empty()) {
    ok = ok && CRT_HIP_OK(hipMalloc(&r.d_mat_index, n_materials * sizeof(uint16_t))) &&
         CRT_HIP_OK(hipMemcpy(r.d_mat_index, mat_index.data(), n_materials * sizeof(uint16_t), hipMemcpyHostToDevice));
    materials = unique_mats.data();
    n_materials = unique_mats.size();
    P.n_materials = (uint32_t)n_materials;
  }
  P.mat_index = r.d_mat_index;
  if (ok && n_materials) {
    ok = CRT_HIP_OK(hipMalloc(&r.d_materials, n_materials * sizeof(CrtMaterial))) &&
         CRT_HIP_OK(hipMemcpy(r.d_materials, materials, n_materials * sizeof(CrtMaterial), hipMemcpyHostToDevice));
  }
  if (ok && n_materials) {  // the vertex code's per-material constants, derived on the device by the vertex code's own functions
    ok = CRT_HIP_OK(hipMalloc(&r.d_mat_derived, n_materials * kKernelBuild.sizeof_material));
    if (ok) {
      hipLaunchKernelGGL(kStageKernels.derive_materials, dim3((unsigned)((n_materials + 255) / 256)), dim3(256), 0, nullptr, r.d_materials,
                         (uint32_t)n_materials, r.d_mat_derived);
      ok = CRT_HIP_OK(hipGetLastError());
    }
  }
  if (ok && n_materials) {  // shade's partition key: one class byte per geom_id
    std::vector<uint8_t> cls(n_materials);
    bool seen[kClasses] = {false, false, false, false};
    for (size_t k = 0; k < n_materials; k++) { cls[k] = material_class(materials[k]); seen[cls[k]] = true; }
    int distinct = 0;
    for (int c = 0; c < kClasses; c++) distinct += seen[c] ? 1 : 0;
    P.partition = distinct > 1 ? 1u : 0u;
    if (knobs.partition >= 0) P.partition = knobs.partition ? 1u : 0u;  // CRT_PARTITION (A/B runs)
    ok = CRT_HIP_OK(hipMalloc(&r.d_mat_class, n_materials)) &&
         CRT_HIP_OK(hipMemcpy(r.d_mat_class, cls.data(), n_materials, hipMemcpyHostToDevice));
  }
  if (ok && n_lights) {
    ok = CRT_HIP_OK(hipMalloc(&r.d_lights, n_lights * sizeof(CrtLight))) &&
         CRT_HIP_OK(hipMemcpy(r.d_lights, lights, n_lights * sizeof(CrtLight), hipMemcpyHostToDevice));
  }
  DevMedium *media_by_id = nullptr;  // the second half of d_media (DevMedium is known here by its size only)
  if (ok && n_materials) {  // interior media of the materials, derived on the device
    uint32_t *d_count = nullptr, h_count = 0;
    ok = CRT_HIP_OK(hipMalloc(&r.d_media, 2 * n_materials * kKernelBuild.sizeof_medium)) && CRT_HIP_OK(hipMalloc(&d_count, 4));
    if (ok) {
      media_by_id = reinterpret_cast<DevMedium *>(reinterpret_cast<char *>(r.d_media) + n_materials * kKernelBuild.sizeof_medium);
      hipLaunchKernelGGL(kStageKernels.build_media, dim3((unsigned)((n_materials + 255) / 256)), dim3(256), 0, nullptr, r.d_materials,
                         (uint32_t)n_materials, r.d_media);
      hipLaunchKernelGGL(kStageKernels.number_media, dim3(1), dim3(kNumberBlock), 0, nullptr, (uint32_t)n_materials, r.d_media,
                         media_by_id, d_count);
      ok = CRT_HIP_OK(hipGetLastError()) && CRT_HIP_OK(hipMemcpy(&h_count, d_count, 4, hipMemcpyDeviceToHost));
      ok = ok && h_count <= kMaxMedia;  // the path state carries a 14-bit medium id
      r.has_media = h_count > 0;
    }
    if (d_count) (void)hipFree(d_count);
  }
  if (!ok) return nullptr;
  {
    bool simple = true;
    for (size_t k = 0; k < n_materials; k++) simple = simple && material_class(materials[k]) <= 1;
    simple = simple && knobs.simple != 0;  // CRT_SIMPLE=0: the general instance (A/B, tests)
    r.in.mats_kind = r.has_media ? 2 : (simple ? 0 : 1);
    // a curve image runs the general instances: no simple-material k_path is built with the rounded-cone arm
    if ((P.scene.cold & kColdCurve) && r.in.mats_kind == 0) r.in.mats_kind = 1;
  }
  P.materials = r.d_materials; P.mat_derived = r.d_mat_derived; P.lights = r.d_lights; P.pixel_index = r.d_pixels;
  P.mat_class = r.d_mat_class;
  P.media = r.d_media; P.media_by_id = media_by_id;
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  // Pipeline by scene (launch_plan.h: PlanInputs, wide_split): small flat triangle scenes gain 4-9 % from
  // the fourth wave per SIMD of the per-stage kernels; an instanced city loses 6 % to their four-entry LDS stack, and a
  // scene of analytic spheres only (openpbr_showcase: next to no traversal, all shading) 1 % to the hit records' round
  // trip (profiles/README.md).
  // select_engine decides, from the image, which engine instance runs it; CRT_WIDE=0/1 (A/B, tests) is a request it
  // honours only where the image can be decoded by what was asked for (never the four-wave kernels on direct words)
  if (select_engine_env(P.scene, r.in.engine, true) != CRT_OK) {
    set_error_text("crt_renderer_new: no traversal-engine instance of this build can decode the scene image");
    return nullptr;
  }
  // ... and, once lanes overlap a batch's launches, every scene prefers one launch per stage: the sphere-only showcase
  // 12 176 -> 13 078 Mray/s (+7.4 %; round 2, one stream: -1 %). The fused kernel remains what small batches and the tails
  // of large ones run.
  PlanInputs &in = r.in;  // what P holds is copied per batch (plan_lane)
  in.cam_compact_build = kKernelBuild.cam_compact; in.shade_pipe_build = kKernelBuild.shade_pipe; in.root_cull_build = kKernelBuild.root_cull;
  in.pipe_mat_max = kKernelBuild.pipe_mat_max;
  // the A/B knobs (crt_internal.h, Knobs)
  in.prefer_stage = knobs.prefer_stage != 0;  // CRT_PREFER_STAGE; unset: every scene does
  in.cam_compact_ok = knobs.cam_compact != 0;
  in.root_cull_knob = knobs.root_cull;
  r.estimate_root_miss_share();
  in.noclassify_from = knobs.noclassify_from;
  in.shade_pipe = knobs.shade_pipe;
  in.slim_state = knobs.slim_state;
  in.camera_trace_knob = knobs.camera_trace;
  in.camera_vertex_knob = knobs.camera_vertex;
  in.camera_trace_build = kKernelBuild.root_cull && kKernelBuild.cam_compact;
  in.no_emitter = table_has_no_emitter(materials, n_materials);  // of the table the kernels read (deduplicated or not)
  in.mat_derived = knobs.mat_derived != 0;
  in.tail_from = knobs.tail_from;
  in.shade_wide = knobs.shade_wide;
  in.force_fused = knobs.fused;
  in.stage_min_paths = knobs.stage_min_paths;
  in.pixel_table_knob = knobs.pixel_table;
  in.cull_root_lds_knob = knobs.cull_root_lds;
  r.build_pixel_table();  // behind every input of the plan above
  r.max_batch_slots = knobs.max_batch_slots;
  r.n_lanes = knobs.lanes < 1 ? 1 : (knobs.lanes > Renderer::kMaxLanes ? Renderer::kMaxLanes : knobs.lanes);
  r.lane_min_paths = knobs.lane_min_paths;
  // Workgroups per CU = queue segments per CU: Renderer::batch_grid.
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) r.cus = prop.multiProcessorCount;
  r.stage_mult = in.engine.wide ? 8 : 3;
  if (knobs.grid_mult > 0) { r.fused_mult = r.stage_mult = knobs.grid_mult; r.mult_forced = 1; }  // CRT_GRID_MULT: tuning knob
  r.last_plan.fused = in.force_fused >= 0 ? in.force_fused != 0 : !in.prefer_stage;  // until the first batch: the scene's preference
  r.last_plan.wide = !r.last_plan.fused && in.engine.wide;
  r.grid = r.batch_grid(0, r.last_plan.fused);
  hold.p = nullptr;
  return R;
}
CrtRenderer *crt_renderer_new(CrtScene *scene, const CrtMaterial *materials, size_t n_materials, const CrtLight *lights,
                              size_t n_lights, const CrtCamera *camera, const CrtRenderSettings *settings,
                              uint32_t tile_rank, uint32_t tile_world) {
  CrtRenderer *R = nullptr;
  (void)abi_guard("crt_renderer_new", [&] {  // nothing unwinds through the ABI: NULL + crt_last_error
    R = renderer_new(scene, materials, n_materials, lights, n_lights, camera, settings, tile_rank, tile_world);
    return (int)CRT_OK;
  });
  return R;
}
void crt_renderer_free(CrtRenderer *r) { delete r; }
size_t crt_renderer_pixel_count(const CrtRenderer *r) { return r ? r->r.pixels.size() : 0; }
int crt_renderer_pixel_indices(const CrtRenderer *r, uint32_t *out) {
  if (!r || !out) return CRT_ERR_BAD_ARG;
  std::memcpy(out, r->r.pixels.data(), r->r.pixels.size() * 4);
  return CRT_OK;
}
int crt_render_samples(CrtRenderer *r, uint32_t sample_begin, uint32_t sample_count, void *stream) {
  if (!r) return CRT_ERR_BAD_ARG;
  return abi_guard("crt_render_samples", [&] { return r->r.render(sample_begin, sample_count, (hipStream_t)stream, nullptr); });
}
// k_volume reads planes a, b and d of camera paths; a CRT_REGEN_FIRST build writes no plane d for them (generate_segment)
// and has shade work them out again, so that A/B build renders no volumes — as it builds neither the root cull nor the
// pipelined shade kernel.
static int renderer_set_volumes(CrtRenderer *r, CrtVolumes *v) {
  Renderer &R = r->r;
  if (v == R.volumes) return CRT_OK;
  if (v && kKernelBuild.regen_first) {
    set_error_text("crt_renderer_set_volumes: a CRT_REGEN_FIRST build holds no volume stage");
    return CRT_ERR_UNSUPPORTED;
  }
  if (v && R.faces) {
    set_error_text("crt_renderer_set_volumes: a per-face texture aggregate is bound; textures together with volumes are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  if (v && R.guiding) {
    set_error_text("crt_renderer_set_volumes: a guiding field is bound; guided renders with volumes are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  VolumesView view;
  if (v) {  // the image is uploaded here, not by the first batch
    const int rc = volumes_device(v, view);
    if (rc != CRT_OK) return rc;
  }
  // nothing of an earlier batch may be in flight when the buffers change shape (the seed plane comes and goes with the
  // binding) or the old aggregate's last reference goes
  if (!CRT_HIP_OK(hipStreamSynchronize(R.last_stream))) return CRT_ERR_NO_DEVICE;
  for (Renderer::Lane &B : R.lanes) {
    if (B.stream) (void)hipStreamSynchronize(B.stream);
    if (B.blob) (void)hipFree(B.blob);
    B.blob = nullptr; B.cap_slots = 0; B.blob_bytes = 0; B.qseed = nullptr; B.fplane = nullptr;
  }
  volumes_retain(v);
  volumes_release(R.volumes);
  R.volumes = v;
  R.vol = VolArgs{view.regions, view.grid, view.n_regions};
  return CRT_OK;
}
int crt_renderer_set_volumes(CrtRenderer *r, CrtVolumes *v) {
  if (!r) return CRT_ERR_BAD_ARG;
  return abi_guard("crt_renderer_set_volumes", [&] { return renderer_set_volumes(r, v); });  // nothing unwinds through the ABI
}
// The FACES instances read plane d of camera paths like every shade instance; a CRT_REGEN_FIRST build has shade work
// camera paths out again in instances of its own, which hold no FACES form: that A/B build renders no textures.
static int renderer_set_face_textures(CrtRenderer *r, CrtFaceTextures *ft) {
  Renderer &R = r->r;
  if (ft == R.faces) return CRT_OK;
  if (ft && kKernelBuild.regen_first) {
    set_error_text("crt_renderer_set_face_textures: a CRT_REGEN_FIRST build holds no textured shade instances");
    return CRT_ERR_UNSUPPORTED;
  }
  if (ft && R.volumes) {
    set_error_text("crt_renderer_set_face_textures: a volume aggregate is bound; textures together with volumes are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  if (ft && R.guiding) {
    set_error_text("crt_renderer_set_face_textures: a guiding field is bound; guided renders with textures are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  dev::FaceView view{};
  if (ft) {
    uint32_t n_geoms = 0, n_materials = 0;
    face_textures_counts(ft, n_geoms, n_materials);
    if (n_geoms > R.scene->n_geoms || n_materials > R.n_materials_given) {
      set_error_text("crt_renderer_set_face_textures: the aggregate binds geometries below %u and materials below %u; the renderer has %u and %u",
                     n_geoms, n_materials, R.scene->n_geoms, R.n_materials_given);
      return CRT_ERR_BAD_ARG;
    }
    const int rc = face_textures_device(ft, view);  // the image is uploaded here, not by the first batch
    if (rc != CRT_OK) return rc;
  }
  // nothing of an earlier batch may be in flight when the buffers change shape (the face record plane comes and goes with
  // the binding) or the old aggregate's last reference goes
  if (!CRT_HIP_OK(hipStreamSynchronize(R.last_stream))) return CRT_ERR_NO_DEVICE;
  for (Renderer::Lane &B : R.lanes) {
    if (B.stream) (void)hipStreamSynchronize(B.stream);
    if (B.blob) (void)hipFree(B.blob);
    B.blob = nullptr; B.cap_slots = 0; B.blob_bytes = 0; B.qseed = nullptr; B.fplane = nullptr;
  }
  face_textures_retain(ft);
  face_textures_release(R.faces);
  R.faces = ft;
  R.face_view = view;
  return CRT_OK;
}
int crt_renderer_set_face_textures(CrtRenderer *r, CrtFaceTextures *ft) {
  if (!r) return CRT_ERR_BAD_ARG;
  return abi_guard("crt_renderer_set_face_textures", [&] { return renderer_set_face_textures(r, ft); });  // nothing unwinds through the ABI
}
// The GUIDED instances read plane d of camera paths like every shade instance; a CRT_REGEN_FIRST build has shade work
// camera paths out again in instances of its own, which hold no GUIDED form: that A/B build renders nothing guided.
static int renderer_set_guiding(CrtRenderer *r, CrtGuiding *g) {
  Renderer &R = r->r;
  if (g == R.guiding) return CRT_OK;
  if (g && kKernelBuild.regen_first) {
    set_error_text("crt_renderer_set_guiding: a CRT_REGEN_FIRST build holds no guided shade instances");
    return CRT_ERR_UNSUPPORTED;
  }
  if (g && R.volumes) {
    set_error_text("crt_renderer_set_guiding: a volume aggregate is bound; guided renders with volumes are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  if (g && R.faces) {
    set_error_text("crt_renderer_set_guiding: a per-face texture aggregate is bound; guided renders with textures are not built");
    return CRT_ERR_UNSUPPORTED;
  }
  dev::GuideView view{};
  if (g) {  // the image is uploaded here, not by the first batch
    const int rc = guiding_device(g, view);
    if (rc != CRT_OK) return rc;
  }
  // nothing of an earlier batch may be in flight when the old field's last reference goes (the buffers keep their shape:
  // a guided batch has no plane of its own)
  if (!CRT_HIP_OK(hipStreamSynchronize(R.last_stream))) return CRT_ERR_NO_DEVICE;
  for (Renderer::Lane &B : R.lanes)
    if (B.stream) (void)hipStreamSynchronize(B.stream);
  guiding_retain(g);
  guiding_release(R.guiding);
  R.guiding = g;
  R.guide_view = view;
  return CRT_OK;
}
int crt_renderer_set_guiding(CrtRenderer *r, CrtGuiding *g) {
  if (!r) return CRT_ERR_BAD_ARG;
  return abi_guard("crt_renderer_set_guiding", [&] { return renderer_set_guiding(r, g); });  // nothing unwinds through the ABI
}
int crt_render_samples_stats(CrtRenderer *r, uint32_t sample_begin, uint32_t sample_count, void *stream,
                             CrtTravStats host_stats[2]) {
  if (!r || !host_stats) return CRT_ERR_BAD_ARG;
  if (r->r.guiding) { set_error_text("crt_render_samples_stats: the stats build does not run guided renders"); return CRT_ERR_UNSUPPORTED; }
  if (r->r.faces) { set_error_text("crt_render_samples_stats: the stats build does not run textured renders"); return CRT_ERR_UNSUPPORTED; }
  if (r->r.volumes) { set_error_text("crt_render_samples_stats: the stats build does not run volume renders"); return CRT_ERR_UNSUPPORTED; }
  CrtTravStats *d = nullptr;
  if (!CRT_HIP_OK(hipMalloc(&d, 2 * sizeof(CrtTravStats)))) return CRT_ERR_NO_DEVICE;
  (void)hipMemsetAsync(d, 0, 2 * sizeof(CrtTravStats), (hipStream_t)stream);
  int rc = abi_guard("crt_render_samples_stats", [&] { return r->r.render(sample_begin, sample_count, (hipStream_t)stream, d); });
  CrtTravStats h[2] = {};
  if (rc == CRT_OK && !CRT_HIP_OK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, (hipStream_t)stream))) rc = CRT_ERR_NO_DEVICE;
  if (!CRT_HIP_OK(hipStreamSynchronize((hipStream_t)stream))) rc = CRT_ERR_NO_DEVICE;
  (void)hipFree(d);
  if (rc == CRT_OK) {
    for (int w = 0; w < 2; w++) {
      for (int k = 0; k < 2; k++) {
        host_stats[w].queries[k] += h[w].queries[k]; host_stats[w].nodes[k] += h[w].nodes[k];
        host_stats[w].leaves[k] += h[w].leaves[k]; host_stats[w].packets[k] += h[w].packets[k];
        host_stats[w].prims[k] += h[w].prims[k];
      }
      host_stats[w].accepted_hits += h[w].accepted_hits; host_stats[w].instance_descents += h[w].instance_descents;
      host_stats[w].rays += h[w].rays;
      for (int k = 0; k < 8; k++) { host_stats[w].phase_waves[k] += h[w].phase_waves[k]; host_stats[w].phase_lanes[k] += h[w].phase_lanes[k]; host_stats[w].phase_cycles[k] += h[w].phase_cycles[k]; }
    }
  }
  return rc;
}
int crt_film_resolve(CrtRenderer *r, float *d_rgb, void *stream) {
  if (!r || !d_rgb) return CRT_ERR_BAD_ARG;
  hipLaunchKernelGGL(kStageKernels.film_out, dim3(r->r.grid), dim3(kBlock), 0, (hipStream_t)stream, r->r.film, r->r.P.n_pix, d_rgb);
  return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE;
}
int crt_film_read(CrtRenderer *r, float *host_rgb) {
  if (!r || !host_rgb) return CRT_ERR_BAD_ARG;
  float *d = nullptr;
  const size_t bytes = (size_t)r->r.P.n_pix * 12;
  if (!CRT_HIP_OK(hipMalloc(&d, bytes))) return CRT_ERR_NO_DEVICE;
  int rc = crt_film_resolve(r, d, r->r.last_stream);
  if (rc == CRT_OK && !CRT_HIP_OK(hipStreamSynchronize(r->r.last_stream))) rc = CRT_ERR_NO_DEVICE;
  if (rc == CRT_OK && !CRT_HIP_OK(hipMemcpy(host_rgb, d, bytes, hipMemcpyDeviceToHost))) rc = CRT_ERR_NO_DEVICE;
  (void)hipFree(d);
  return rc;
}
int crt_film_clear(CrtRenderer *r, void *stream) {
  if (!r) return CRT_ERR_BAD_ARG;
  bool ok = CRT_HIP_OK(hipMemsetAsync(r->r.film, 0, (size_t)r->r.P.n_pix * 16, (hipStream_t)stream));
  for (Renderer::Lane &B : r->r.lanes) ok = ok && CRT_HIP_OK(hipMemsetAsync(B.C, 0, sizeof(Counters), (hipStream_t)stream));
  if (ok && r->r.d_state) {
    ok = CRT_HIP_OK(hipMemsetAsync(r->r.d_state, 0, (size_t)r->r.P.n_pix * 4, (hipStream_t)stream)) &&
         CRT_HIP_OK(hipMemsetAsync(r->r.d_pstats, 0, (size_t)r->r.P.n_pix * sizeof(PixelStats), (hipStream_t)stream));
    r->r.n_act = r->r.P.n_pix;
  }
  return ok ? CRT_OK : CRT_ERR_NO_DEVICE;
}
int crt_render_stats(CrtRenderer *r, CrtRayStats *out) {
  if (!r || !out) return CRT_ERR_BAD_ARG;
  struct { uint32_t err, pad; unsigned long long stats[8]; } h;  // the head of Counters
  static_assert(offsetof(Counters, seg) == sizeof h, "Counters head layout");
  if (!CRT_HIP_OK(hipStreamSynchronize(r->r.last_stream))) return CRT_ERR_NO_DEVICE;
  unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t err = 0;
  for (const Renderer::Lane &B : r->r.lanes) {  // the lanes of a batch count their own rays
    if (!CRT_HIP_OK(hipMemcpy(&h, B.C, sizeof h, hipMemcpyDeviceToHost))) return CRT_ERR_NO_DEVICE;
    for (int k = 0; k < 8; k++) sum[k] += h.stats[k];
    err |= h.err;
  }
  out->camera_rays = sum[0]; out->closest_hit = sum[1]; out->shadow_rays = sum[2];
  out->vertices = sum[3]; out->rr_tested = sum[4]; out->rr_killed = sum[5];
  out->ended_escaped = sum[6]; out->ended_depth = sum[7];
  return err ? CRT_ERR_STACK : CRT_OK;
}
size_t crt_renderer_active_pixels(const CrtRenderer *r) { return r ? (r->r.variance_threshold > 0.0f ? r->r.n_act : r->r.P.n_pix) : 0; }
int crt_renderer_sample_counts(CrtRenderer *r, uint32_t *host_out) {
  if (!r || !host_out) return CRT_ERR_BAD_ARG;
  if (!r->r.d_state) return CRT_ERR_UNSUPPORTED;
  if (!CRT_HIP_OK(hipStreamSynchronize(r->r.last_stream))) return CRT_ERR_NO_DEVICE;
  if (!CRT_HIP_OK(hipMemcpy(host_out, r->r.d_state, (size_t)r->r.P.n_pix * 4, hipMemcpyDeviceToHost))) return CRT_ERR_NO_DEVICE;
  for (size_t k = 0; k < r->r.P.n_pix; k++) host_out[k] &= 0x7fffffffu;
  return CRT_OK;
}
int crt_renderer_shade_class_stats(CrtRenderer *r, int enable, uint64_t out_waves[4], uint64_t out_lanes[4]) {
  if (!r) return CRT_ERR_BAD_ARG;
  Renderer &R = r->r;
  if (out_waves && out_lanes) {
    unsigned long long h[8];
    if (!CRT_HIP_OK(hipStreamSynchronize(R.last_stream))) return CRT_ERR_NO_DEVICE;
    for (int c = 0; c < 4; c++) out_waves[c] = out_lanes[c] = 0;
    for (Renderer::Lane &B : R.lanes) {
      if (!CRT_HIP_OK(hipMemcpy(h, B.C->cls_waves, sizeof h, hipMemcpyDeviceToHost))) return CRT_ERR_NO_DEVICE;
      if (!CRT_HIP_OK(hipMemset(B.C->cls_waves, 0, sizeof h))) return CRT_ERR_NO_DEVICE;
      for (int c = 0; c < 4; c++) { out_waves[c] += h[c]; out_lanes[c] += h[4 + c]; }
    }
  }
  if (enable >= 0) R.P.class_stats = enable ? 1u : 0u;
  return CRT_OK;
}
int crt_renderer_lanes(const CrtRenderer *r) { return r ? r->r.last_lanes : 0; }
int crt_renderer_set_lanes(CrtRenderer *r, int lanes) {
  if (!r) return CRT_ERR_BAD_ARG;
  r->r.n_lanes = lanes < 1 ? 1 : (lanes > Renderer::kMaxLanes ? Renderer::kMaxLanes : lanes);
  return r->r.n_lanes;
}
int crt_renderer_pipeline(const CrtRenderer *r, uint32_t out[3]) {
  if (!r || !out) return CRT_ERR_BAD_ARG;
  const LaunchPlan &plan = r->r.last_plan;  // every bit below is a per-stage one: plan_launches sets none of them on a fused plan
  out[0] = plan.fused ? 1u : 0u;
  out[1] = (plan.wide ? 1u : 0u) | (plan.shade_piped() ? 2u : 0u) | (plan.root_cull ? 4u : 0u) | (plan.slim_state ? 8u : 0u) |
           (plan.volumes ? 16u : 0u) | (plan.camera_trace ? 32u : 0u) | (plan.camera_vertex ? 64u : 0u) |
           (plan.pixel_table ? 128u : 0u) | (plan.cull_root_lds ? 256u : 0u) | (plan.faces ? 512u : 0u) | (plan.guided ? 1024u : 0u);
  out[2] = (uint32_t)r->r.grid;
  return CRT_OK;
}
int crt_renderer_profile(CrtRenderer *r, int enable) {
  if (!r) return CRT_ERR_BAD_ARG;
  r->r.drain_events();
  r->r.profile = enable != 0;
  for (int k = 0; k < 4; k++) { r->r.prof_ms[k] = 0; r->r.prof_launches[k] = 0; }
  return CRT_OK;
}
int crt_renderer_profile_read(CrtRenderer *r, double out_ms[4], uint64_t out_launches[4]) {
  if (!r || !out_ms || !out_launches) return CRT_ERR_BAD_ARG;
  r->r.drain_events();
  for (int k = 0; k < 4; k++) { out_ms[k] = r->r.prof_ms[k]; out_launches[k] = r->r.prof_launches[k]; }
  return CRT_OK;
}

}  // extern "C"
