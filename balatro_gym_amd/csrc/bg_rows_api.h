// bg_rows_api.h -- the stateless half of the C ABI: every entry point that takes no bg_handle (the measurement hooks, the batch operators and the
// record learners).  Included by bg_lib.hip (one translation unit) inside its extern "C" block, behind the handle API: g_create_err, bg_rows_args and
// the kernel headers are in scope.  A new entry point checks its arguments into one `bad` verdict, opens with bg_op_begin and launches through
// bg_op_run ("Source-only changes to the engines").
#ifndef BG_ROWS_API_H
#define BG_ROWS_API_H

// ---- operator-level entry points (no handle: they run on the CURRENT device, on caller-owned device buffers) ----
#define BG_HIP0(call)                                                                                  \
  do {                                                                                                 \
    hipError_t _e = (call);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      g_create_err = std::string(#call) + ": " + hipGetErrorString(_e);                                \
      return BG_E_HIP;                                                                                 \
    }                                                                                                  \
  } while (0)

// ---- measurement hook: streaming copy (bench.py's `peak_measured`: what this GPU's HBM sustains for a plain 16-byte-per-lane
// copy, the yardstick SURVEY 8(d) asks the roofline fraction to be quoted against beside the 8 TB/s nominal) ----
// Shape from a sweep on the MI355X (tools/micro/copybw.hip, profiles/r03_copybw.txt): ONE pass per workgroup (no grid-stride loop), four
// 16-byte pieces per lane, non-temporal loads and stores: 6.5 TB/s read + written at 1 GiB (the guide's float4 copy: 6.29; the
// grid-stride kernel of rounds 1-2: 5.1-5.6).  A plain one-pass fill writes 6.8 TB/s.
__global__ __launch_bounds__(256) void bg_stream_copy_kernel(const bg_cp_u32x4* __restrict__ src, bg_cp_u32x4* __restrict__ dst, size_t n16) {
  const size_t i = (size_t)blockIdx.x * 256 * 4 + threadIdx.x;
  bg_cp_u32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) if (i + (size_t)k * 256 < n16) v[k] = __builtin_nontemporal_load(&src[i + (size_t)k * 256]);
#pragma unroll
  for (int k = 0; k < 4; k++) if (i + (size_t)k * 256 < n16) __builtin_nontemporal_store(v[k], &dst[i + (size_t)k * 256]);
}
int bg_bench_copy(const void* src_dev, void* dst_dev, uint64_t bytes, int iters, double* gbps_out, void* stream) {
  if (!src_dev || !dst_dev || !gbps_out || bytes < 16 || iters < 1 || ((uintptr_t)src_dev & 15) || ((uintptr_t)dst_dev & 15)) { g_create_err = "bg_bench_copy: bad arguments"; return BG_E_ARG; }
  hipStream_t s = (hipStream_t)stream;
  const size_t n16 = bytes / 16;
  const unsigned grid = (unsigned)((n16 + 1023) / 1024);
  hipEvent_t a, b;
  BG_HIP0(hipEventCreate(&a)); BG_HIP0(hipEventCreate(&b));
  for (int i = 0; i < 2; i++) hipLaunchKernelGGL(bg_stream_copy_kernel, dim3(grid), dim3(256), 0, s, (const bg_cp_u32x4*)src_dev, (bg_cp_u32x4*)dst_dev, n16); // warm-up
  BG_HIP0(hipEventRecord(a, s));
  for (int i = 0; i < iters; i++) hipLaunchKernelGGL(bg_stream_copy_kernel, dim3(grid), dim3(256), 0, s, (const bg_cp_u32x4*)src_dev, (bg_cp_u32x4*)dst_dev, n16);
  BG_HIP0(hipEventRecord(b, s));
  BG_HIP0(hipGetLastError());
  BG_HIP0(hipEventSynchronize(b));
  float ms = 0;
  BG_HIP0(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  *gbps_out = ms > 0 ? 2.0 * (double)(n16 * 16) * iters / (ms * 1e-3) / 1e9 : 0.0; // bytes read + bytes written
  return 0;
}

// write-only twin: the step engine's traffic is ~80 % stores (the record of every step), so the store bandwidth is its real ceiling
__global__ __launch_bounds__(256) void bg_stream_fill_kernel(uint4* __restrict__ dst, size_t n16, uint32_t seed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) dst[i] = make_uint4(seed, (uint32_t)i, 0u, seed ^ (uint32_t)i);
}
int bg_bench_fill(void* dst_dev, uint64_t bytes, int iters, double* gbps_out, void* stream) {
  if (!dst_dev || !gbps_out || bytes < 16 || iters < 1 || ((uintptr_t)dst_dev & 15)) { g_create_err = "bg_bench_fill: bad arguments"; return BG_E_ARG; }
  hipStream_t s = (hipStream_t)stream;
  const size_t n16 = bytes / 16;
  const unsigned grid = (unsigned)((n16 + 255) / 256);
  hipEvent_t a, b;
  BG_HIP0(hipEventCreate(&a)); BG_HIP0(hipEventCreate(&b));
  for (int i = 0; i < 2; i++) hipLaunchKernelGGL(bg_stream_fill_kernel, dim3(grid), dim3(256), 0, s, (uint4*)dst_dev, n16, 0u); // warm-up
  BG_HIP0(hipEventRecord(a, s));
  for (int i = 0; i < iters; i++) hipLaunchKernelGGL(bg_stream_fill_kernel, dim3(grid), dim3(256), 0, s, (uint4*)dst_dev, n16, (uint32_t)i + 1u);
  BG_HIP0(hipEventRecord(b, s));
  BG_HIP0(hipGetLastError());
  BG_HIP0(hipEventSynchronize(b));
  float ms = 0;
  BG_HIP0(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  *gbps_out = ms > 0 ? (double)(n16 * 16) * iters / (ms * 1e-3) / 1e9 : 0.0; // bytes written
  return 0;
}

// kernel-only time of a batch op (the A/B of the two lane mappings): events on the caller's stream around the launch
struct BgOpTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  int begin(float* out, hipStream_t s) { on = out != nullptr; if (!on) return 0; BG_HIP0(hipEventCreate(&a)); BG_HIP0(hipEventCreate(&b)); BG_HIP0(hipEventRecord(a, s)); return 0; }
  void mark(hipStream_t s) { if (on) (void)hipEventRecord(b, s); }
  int end(float* out) { if (!on) return 0; BG_HIP0(hipEventSynchronize(b)); BG_HIP0(hipEventElapsedTime(out, a, b)); (void)hipEventDestroy(a); (void)hipEventDestroy(b); return 0; }
};

// The scaffold of a stateless entry point, in the two steps that every one of them takes around its own empty-shape return:
//   if (int rc = bg_op_begin("bg_name: ", bad, kernel_ms_out)) return rc;   // the verdict of the argument checks: refused, or the time zeroed
//   if (m == 0) return 0;                                                    // (an entry point that clears an output for an empty shape does so here)
//   return bg_op_run(kernel_ms_out, s, [&] { ...launches... });             // the launches between the timer's events, then hipGetLastError
static int bg_op_begin(const char* who, const char* bad, float* kernel_ms_out) {
  if (bad) { g_create_err = std::string(who) + bad; return BG_E_ARG; }
  if (kernel_ms_out) *kernel_ms_out = 0.f;
  return 0;
}
extern "C++" {   // (templates: the header is read inside bg_lib.hip's extern "C" block)
template <class F>
static int bg_op_run(float* kernel_ms_out, hipStream_t s, F launches) {
  BgOpTimer tm;
  int rc = tm.begin(kernel_ms_out, s);
  if (rc) return rc;
  launches();
  tm.mark(s);
  BG_HIP0(hipGetLastError());
  return tm.end(kernel_ms_out);
}
// two run-time booleans -> launch(A, B) as constants, in the style of bg_enc_dispatch (bg_encode.h)
template <class F>
static void bg_bool_dispatch(bool a, bool b, F launch) {
  if (a) { if (b) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
  else { if (b) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
}
// an output (nullable) is the same pointer as an input or as another output
template <size_t NI, size_t NO>
static bool bg_alias(const void* const (&ins)[NI], const void* const (&outs)[NO]) {
  bool alias = false;
  for (size_t o = 0; o < NO; o++) {
    if (!outs[o]) continue;
    for (size_t i = 0; i < NI; i++) alias = alias || outs[o] == ins[i];
    for (size_t q = o + 1; q < NO; q++) alias = alias || outs[o] == outs[q];
  }
  return alias;
}
}   // extern "C++"

int bg_classify_batch_ex(const uint8_t* cards_dev, const uint8_t* n_dev, uint8_t* hand_type_dev, int64_t m, int lanes_per_case,
                         float* kernel_ms_out, void* stream) {
  const char* bad = nullptr;
  if (!cards_dev || !n_dev || !hand_type_dev || m < 0 || ((uintptr_t)cards_dev & 7) || (lanes_per_case != 1 && lanes_per_case != 8))
    bad = "bg_classify_batch: bad arguments (cards_dev must be 8-byte aligned, lanes_per_case 1 or 8)";
  if (int rc = bg_op_begin("", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (lanes_per_case == 1)
      hipLaunchKernelGGL(bg_classify_batch_kernel, dim3((unsigned)((m + BG_BLOCK - 1) / BG_BLOCK)), dim3(BG_BLOCK), 0, s, cards_dev, n_dev, hand_type_dev, (long long)m);
    else
      hipLaunchKernelGGL(bg_classify_batch_l8_kernel, dim3((unsigned)((m * 8 + BG_BLOCK - 1) / BG_BLOCK)), dim3(BG_BLOCK), 0, s, cards_dev, n_dev, hand_type_dev, (long long)m);
  });
}
int bg_classify_batch(const uint8_t* cards_dev, const uint8_t* n_dev, uint8_t* hand_type_dev, int64_t m, void* stream) {
  return bg_classify_batch_ex(cards_dev, n_dev, hand_type_dev, m, 1, nullptr, stream);
}

// packed records -> network input (bg_encode.h).  The store path follows the alignment of the caller's matrix.
int bg_encode_cols(int layout) { const int d = bg_enc_cols(layout); return d > 0 ? d : BG_E_ARG; }

// the output matrix of bg_encode_rows, bg_encode_rows_ex and bg_norm_obs_rows: D columns of es bytes.  optional: NULL asks for no matrix (bg_norm_obs_rows)
static const char* bg_enc_out_args(const void* out_dev, uint64_t out_stride_elems, uint64_t es, int D, bool optional) {
  if (optional && !out_dev) return nullptr;
  if (!out_dev || ((uintptr_t)out_dev & (es - 1))) return optional ? "out_dev must be aligned to its element type" : "out_dev must be a device pointer aligned to its element type";
  if (out_stride_elems < (uint64_t)D || out_stride_elems > 0xffffffffull) return "out_stride_elems must be >= the layout's column count";
  return nullptr;
}
// what bg_encode_rows and bg_encode_rows_ex check first: D = bg_enc_cols(layout), the element type, the number of output rows
static const char* bg_enc_shape_args(int D, int out_dtype, int64_t m) {
  if (D < 0) return "layout must be BG_ENC_PRODUCED, BG_ENC_FIXED or BG_ENC_EXTRACTOR";
  if (out_dtype != BG_ENC_F32 && out_dtype != BG_ENC_BF16) return "out_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  if (m < 0 || m > (int64_t)BG_ENC_RECS * 0x7fffffffll) return "m out of range";
  return nullptr;
}

int bg_encode_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t m, int layout, int out_dtype, void* out_dev,
                   uint64_t out_stride_elems, float* kernel_ms_out, void* stream) {
  const int D = bg_enc_cols(layout);
  const uint64_t es = out_dtype == BG_ENC_F32 ? 4u : 2u;
  const char* bad = bg_enc_shape_args(D, out_dtype, m);
  if (bad) {}
  else if (const char* r = bg_rows_args(rows_dev, row_stride_bytes)) bad = r;
  else if (const char* r = bg_enc_out_args(out_dev, out_stride_elems, es, D, false)) bad = r;
  if (int rc = bg_op_begin("bg_encode_rows: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const int st = bg_enc_store_path(out_dev, out_stride_elems, es, D);
  const unsigned grid = (unsigned)((m + BG_ENC_RECS - 1) / BG_ENC_RECS);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_enc_dispatch<BG_ENC_EXTRACTOR>(layout, out_dtype, st, [&](auto L, auto T, auto S) {
      hipLaunchKernelGGL((bg_encode_kernel<L(), T(), S()>), dim3(grid), dim3(BG_ENC_BLOCK), 0, s, rows_dev, row_stride_bytes, (long long)m, out_dev, out_stride_elems);
    });
  });
}

// packed records -> PPO's scans along K (bg_gae.h): advantages / returns, and per-episode reward sums / lengths with a per-env carry
static const char* bg_scan_args(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N) {
  if (K < 0 || N < 0 || N > (int64_t)BG_GAE_ENVS * 0x7fffffffll) return "K / N out of range";
  return bg_rows_args(rows_dev, row_stride_bytes);
}

int bg_gae_rows_ex(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, const float* values_dev, const float* last_values_dev,
                   double gamma, double gae_lambda, float* advantages_dev, float* returns_dev, const double* rewards_dev, float* kernel_ms_out, void* stream) {
  const char* const who = rewards_dev ? "bg_gae_rows_ex: " : "bg_gae_rows: ";
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (!bad && (!values_dev || !last_values_dev || !advantages_dev)) bad = "values_dev, last_values_dev and advantages_dev must be device pointers";
  else if (!bad && (((uintptr_t)values_dev | (uintptr_t)last_values_dev | (uintptr_t)advantages_dev | (uintptr_t)returns_dev) & 3)) bad = "float arrays must be 4-byte aligned";
  else if (!bad && ((uintptr_t)rewards_dev & 7)) bad = "rewards_dev must be 8-byte aligned";
  else if (!bad && (advantages_dev == values_dev || returns_dev == values_dev || (returns_dev && returns_dev == advantages_dev))) bad = "advantages_dev / returns_dev must not be the same pointer as values_dev or as each other";
  else if (!bad && rewards_dev && ((const void*)rewards_dev == (const void*)advantages_dev || (const void*)rewards_dev == (const void*)returns_dev)) bad = "advantages_dev / returns_dev must not be the same pointer as rewards_dev";
  if (int rc = bg_op_begin(who, bad, kernel_ms_out)) return rc;
  if (K == 0 || N == 0) return 0;
  const unsigned grid = (unsigned)((N + BG_GAE_ENVS - 1) / BG_GAE_ENVS);
  const float g = bg_gae_g(gamma), gl = bg_gae_gl(gamma, gae_lambda);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_bool_dispatch(returns_dev != nullptr, rewards_dev != nullptr, [&](auto R, auto W) {
      hipLaunchKernelGGL((bg_gae_kernel<R(), W()>), dim3(grid), dim3(BG_GAE_BLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, values_dev, last_values_dev, g, gl, advantages_dev, returns_dev, rewards_dev);
    });
  });
}
int bg_gae_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, const float* values_dev, const float* last_values_dev,
                double gamma, double gae_lambda, float* advantages_dev, float* returns_dev, float* kernel_ms_out, void* stream) {
  return bg_gae_rows_ex(rows_dev, row_stride_bytes, K, N, values_dev, last_values_dev, gamma, gae_lambda, advantages_dev, returns_dev, nullptr, kernel_ms_out, stream);
}

int bg_episode_stats_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, double* ep_return_carry_dev, int32_t* ep_len_carry_dev,
                          double* ep_return_dev, int32_t* ep_len_dev, float* kernel_ms_out, void* stream) {
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (!bad && (!ep_return_carry_dev || !ep_len_carry_dev)) bad = "ep_return_carry_dev and ep_len_carry_dev must be device pointers";
  else if (!bad && ((((uintptr_t)ep_return_carry_dev | (uintptr_t)ep_return_dev) & 7) || (((uintptr_t)ep_len_carry_dev | (uintptr_t)ep_len_dev) & 3))) bad = "float64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned";
  else if (!bad && (ep_return_dev == ep_return_carry_dev || ep_len_dev == ep_len_carry_dev)) bad = "ep_return_dev / ep_len_dev must not be the same pointer as their carry";
  if (int rc = bg_op_begin("bg_episode_stats_rows: ", bad, kernel_ms_out)) return rc;
  if (K == 0 || N == 0) return 0;
  const unsigned grid = (unsigned)((N + BG_GAE_ENVS - 1) / BG_GAE_ENVS);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_bool_dispatch(ep_return_dev != nullptr, ep_len_dev != nullptr, [&](auto R, auto L) {
      hipLaunchKernelGGL((bg_episode_stats_kernel<R(), L()>), dim3(grid), dim3(BG_GAE_BLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, ep_return_carry_dev, ep_len_carry_dev, ep_return_dev, ep_len_dev);
    });
  });
}

// packed records -> the ended episodes of a rollout (bg_ends.h): the report, and the curriculum's state advanced per env in step order
int bg_episode_ends_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, int64_t* report_dev, const bg_curriculum* cur,
                         float* kernel_ms_out, void* stream) {
  static_assert(BG_ENDS_ENVS == BG_GAE_ENVS, "bg_scan_args bounds N by the grid of a 64-env workgroup");
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (!bad && (!report_dev || ((uintptr_t)report_dev & 7))) bad = "report_dev must be an 8-byte aligned device pointer to int64 [BG_ENDS_WORDS]";
  else if (!bad && cur) {
    if (!cur->cap_dev || !cur->hist_dev || !cur->count_dev || !cur->at_level_dev || !cur->raised_dev) bad = "cur: cap_dev, hist_dev, count_dev, at_level_dev and raised_dev must all be device pointers";
    else if ((((uintptr_t)cur->cap_dev | (uintptr_t)cur->at_level_dev) & 3) || ((uintptr_t)cur->hist_dev & 1) || ((uintptr_t)cur->count_dev & 7)) bad = "cur: int32 arrays must be 4-byte aligned, hist_dev 2-byte, count_dev 8-byte";
    else if (cur->window < 1) bad = "cur: window must be >= 1";
    else if (cur->increment < 1 || cur->increment > BG_ENDS_CAP_MAX) bad = "cur: increment must be in 1..255";
    else if (!std::isfinite(cur->threshold)) bad = "cur: threshold must be finite";
  }
  if (int rc = bg_op_begin("bg_episode_ends_rows: ", bad, kernel_ms_out)) return rc;
  hipStream_t s = (hipStream_t)stream;
  BG_HIP0(hipMemsetAsync(report_dev, 0, BG_ENDS_WORDS * sizeof(int64_t), s));
  if (K == 0 || N == 0) {
    if (cur && N > 0) BG_HIP0(hipMemsetAsync(cur->raised_dev, 0, (size_t)N, s));   // (no step: no cap rose)
    return 0;
  }
  const unsigned grid = (unsigned)((N + BG_ENDS_ENVS - 1) / BG_ENDS_ENVS);
  return bg_op_run(kernel_ms_out, s, [&] {
    if (cur) hipLaunchKernelGGL((bg_episode_ends_kernel<true>), dim3(grid), dim3(BG_ENDS_BLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, (unsigned long long*)report_dev, *cur);
    else hipLaunchKernelGGL((bg_episode_ends_kernel<false>), dim3(grid), dim3(BG_ENDS_BLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, (unsigned long long*)report_dev, bg_curriculum{});
  });
}

// packed records -> VecNormalize (bg_norm.h).  Workspace, in doubles: [K * chunks * 306] partial (mean, M2) per (step, 256-env chunk), [K * 306] batch
// moments (when the caller does not take them), [K * 306] (mean, sqrt(var + epsilon)) per step for the normalising pass.  The reward call's needs -- 2 per
// (step, 64-env chunk), 2 + 1 per step -- are smaller at every shape.
static uint64_t bg_norm_chunks(int64_t N) { return ((uint64_t)N + BG_NORM_CHUNK - 1) / BG_NORM_CHUNK; }
static uint64_t bg_norm_rchunks(int64_t N) { return ((uint64_t)N + BG_NORM_RBLOCK - 1) / BG_NORM_RBLOCK; }
uint64_t bg_norm_workspace_bytes(int K, int64_t N) {
  if (K <= 0 || N <= 0) return 0;
  return ((uint64_t)K * bg_norm_chunks(N) + 2u * (uint64_t)K) * (2u * BG_NORM_COLS) * sizeof(double);
}
static_assert(2 * (BG_NORM_CHUNK / BG_NORM_RBLOCK) + 3 <= 2 * BG_NORM_COLS, "the reward call fits the workspace of the observation call");

int bg_norm_obs_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, int layout, int out_dtype, double* mean_dev, double* var_dev,
                     double* count_dev, int update, double epsilon, double clip_obs, void* out_dev, uint64_t out_stride_elems, double* moments_dev,
                     void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const int D = layout == BG_ENC_PRODUCED || layout == BG_ENC_FIXED ? bg_enc_cols(layout) : -1;
  const uint64_t es = out_dtype == BG_ENC_F32 ? 4u : 2u;
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (bad) {}
  else if (D < 0) bad = "layout must be BG_ENC_PRODUCED or BG_ENC_FIXED (VecNormalize wraps the env's keys, not the extractor's tensors)";
  else if (out_dtype != BG_ENC_F32 && out_dtype != BG_ENC_BF16) bad = "out_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  else if ((uint64_t)K * (uint64_t)N > (uint64_t)BG_ENC_RECS * 0x7fffffffull) bad = "K * N out of range";
  else if (!mean_dev || !var_dev || !count_dev || (((uintptr_t)mean_dev | (uintptr_t)var_dev | (uintptr_t)count_dev | (uintptr_t)moments_dev) & 7)) bad = "mean_dev, var_dev and count_dev must be 8-byte aligned device pointers (moments_dev 8-byte aligned)";
  else if (mean_dev == var_dev || mean_dev == count_dev || var_dev == count_dev) bad = "mean_dev, var_dev and count_dev must not be the same pointer";
  else if (const char* r = bg_enc_out_args(out_dev, out_stride_elems, es, D, true)) bad = r;
  else if (!update && moments_dev) bad = "moments_dev must be NULL when update == 0 (no batch moments are taken)";
  else if (!update && !out_dev) bad = "update == 0 with out_dev NULL asks for nothing";
  else if (!(epsilon == epsilon) || !(clip_obs == clip_obs)) bad = "epsilon and clip_obs must not be NaN";
  else if (K > 0 && N > 0 && (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < bg_norm_workspace_bytes(K, N))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_norm_workspace_bytes(K, N) bytes";
  else if (out_dev && ((void*)mean_dev == out_dev || (void*)var_dev == out_dev || (void*)moments_dev == out_dev || workspace_dev == out_dev || (const void*)rows_dev == out_dev)) bad = "out_dev must not be the same pointer as an input or another output";
  if (int rc = bg_op_begin("bg_norm_obs_rows: ", bad, kernel_ms_out)) return rc;
  if (K == 0 || N == 0) return 0;
  const uint64_t chunks = bg_norm_chunks(N);
  double* const part = (double*)workspace_dev;
  double* const mom_ws = part + (uint64_t)K * chunks * (2 * BG_NORM_COLS);
  double* const stat = mom_ws + (uint64_t)K * (2 * BG_NORM_COLS);
  double* const mom = moments_dev ? moments_dev : mom_ws;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (update) {
      hipLaunchKernelGGL(bg_norm_obs_partials, dim3((unsigned)(chunks * (uint64_t)K)), dim3(BG_NORM_PBLOCK), 0, s, rows_dev, row_stride_bytes, (long long)N, (long long)chunks, part);
      hipLaunchKernelGGL(bg_norm_obs_combine, dim3((unsigned)K), dim3(BG_NORM_PBLOCK), 0, s, part, (long long)N, (long long)chunks, mom);
      hipLaunchKernelGGL((bg_norm_obs_chain<true>), dim3(1), dim3(BG_NORM_PBLOCK), 0, s, mom, K, (double)N, epsilon, mean_dev, var_dev, count_dev, stat);
    } else if (out_dev)
      hipLaunchKernelGGL((bg_norm_obs_chain<false>), dim3(1), dim3(BG_NORM_PBLOCK), 0, s, mom, K, (double)N, epsilon, mean_dev, var_dev, count_dev, stat);
    if (out_dev) {
      const long long m = (long long)K * (long long)N;
      const int st = bg_enc_store_path(out_dev, out_stride_elems, es, D);
      const unsigned grid = (unsigned)((m + BG_ENC_RECS - 1) / BG_ENC_RECS);
      const size_t sstride = update ? 2 * BG_NORM_COLS : 0;
      bg_enc_dispatch<BG_ENC_FIXED>(layout, out_dtype, st, [&](auto L, auto T, auto S) {
        hipLaunchKernelGGL((bg_norm_obs_kernel<L(), T(), S()>), dim3(grid), dim3(BG_ENC_BLOCK), 0, s, rows_dev, row_stride_bytes, m, (long long)N, stat, sstride, clip_obs, out_dev, out_stride_elems);
      });
    }
  });
}

// bg_encode_rows / frozen bg_norm_obs_rows for the rows a minibatch names: the GATHER variants of their kernels (bg_encode.h, bg_norm.h).  Without an
// index and without statistics it IS bg_encode_rows; statistics without an index run the GATHER variant with the identity (no workspace to hold
// sqrt(var + epsilon): the workgroups take the roots themselves).
int bg_encode_rows_ex(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, int layout, int out_dtype,
                      const double* mean_dev, const double* var_dev, double epsilon, double clip_obs, void* out_dev, uint64_t out_stride_elems,
                      float* kernel_ms_out, void* stream) {
  const int D = bg_enc_cols(layout);
  const uint64_t es = out_dtype == BG_ENC_F32 ? 4u : 2u;
  const bool norm = mean_dev || var_dev;
  const char* bad = bg_enc_shape_args(D, out_dtype, m);
  if (bad) {}
  else if (store_rows < 0) bad = "store_rows must be >= 0";
  else if (index_dev && store_rows > 0x7fffffffll) bad = "store_rows must be in [0, 2**31) when index_dev is given";
  else if (!index_dev && m > store_rows) bad = "m must be <= store_rows when index_dev is NULL";
  else if (const char* r = bg_rows_args(rows_dev, row_stride_bytes)) bad = r;
  else if ((uintptr_t)index_dev & 3) bad = "index_dev must be 4-byte aligned";
  else if (norm && (!mean_dev || !var_dev)) bad = "mean_dev and var_dev go together: both or neither";
  else if (norm && layout == BG_ENC_EXTRACTOR) bad = "statistics need layout BG_ENC_PRODUCED or BG_ENC_FIXED (VecNormalize wraps the env's keys, not the extractor's tensors)";
  else if (norm && (((uintptr_t)mean_dev | (uintptr_t)var_dev) & 7)) bad = "mean_dev and var_dev must be 8-byte aligned";
  else if (norm && mean_dev == var_dev) bad = "mean_dev and var_dev must not be the same pointer";
  else if (norm && !(epsilon >= 0.0 && epsilon <= 1.7976931348623157e308 && clip_obs >= 0.0 && clip_obs <= 1.7976931348623157e308)) bad = "epsilon and clip_obs must be finite and >= 0 when statistics are given";
  else if (const char* r = bg_enc_out_args(out_dev, out_stride_elems, es, D, false)) bad = r;
  else if (out_dev == (const void*)rows_dev || out_dev == (const void*)index_dev || out_dev == (const void*)mean_dev || out_dev == (const void*)var_dev) bad = "out_dev must not be the same pointer as an input";
  if (int rc = bg_op_begin("bg_encode_rows_ex: ", bad, kernel_ms_out)) return rc;
  if (!index_dev && !norm) return bg_encode_rows(rows_dev, row_stride_bytes, m, layout, out_dtype, out_dev, out_stride_elems, kernel_ms_out, stream);
  if (m == 0) return 0;
  const int st = bg_enc_store_path(out_dev, out_stride_elems, es, D);
  const unsigned grid = (unsigned)((m + BG_ENC_RECS - 1) / BG_ENC_RECS);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (norm)
      bg_enc_dispatch<BG_ENC_FIXED>(layout, out_dtype, st, [&](auto L, auto T, auto S) {
        hipLaunchKernelGGL((bg_norm_obs_gather_kernel<L(), T(), S()>), dim3(grid), dim3(BG_ENC_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, mean_dev, var_dev, epsilon, clip_obs, out_dev, out_stride_elems);
      });
    else
      bg_enc_dispatch<BG_ENC_EXTRACTOR>(layout, out_dtype, st, [&](auto L, auto T, auto S) {
        hipLaunchKernelGGL((bg_encode_gather_kernel<L(), T(), S()>), dim3(grid), dim3(BG_ENC_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, out_dev, out_stride_elems);
      });
  });
}

int bg_norm_reward_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, double* returns_carry_dev, double* ret_stats_dev, int update,
                        double gamma, double epsilon, double clip_reward, double* rewards_dev, double* moments_dev, void* workspace_dev,
                        uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (bad) {}
  else if ((uint64_t)K * (uint64_t)N > 256ull * 0x7fffffffull) bad = "K * N out of range";
  else if (!ret_stats_dev || (update && !returns_carry_dev)) bad = "ret_stats_dev (and, with update != 0, returns_carry_dev) must be device pointers";
  else if (((uintptr_t)returns_carry_dev | (uintptr_t)ret_stats_dev | (uintptr_t)rewards_dev | (uintptr_t)moments_dev) & 7) bad = "float64 arrays must be 8-byte aligned";
  else if (!update && moments_dev) bad = "moments_dev must be NULL when update == 0 (no batch moments are taken)";
  else if (!update && !rewards_dev) bad = "update == 0 with rewards_dev NULL asks for nothing";
  else if (!(gamma == gamma) || !(epsilon == epsilon) || !(clip_reward == clip_reward)) bad = "gamma, epsilon and clip_reward must not be NaN";
  else if (K > 0 && N > 0 && (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < bg_norm_workspace_bytes(K, N))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_norm_workspace_bytes(K, N) bytes";
  else if (rewards_dev && (rewards_dev == returns_carry_dev || rewards_dev == ret_stats_dev || rewards_dev == moments_dev || (void*)rewards_dev == workspace_dev || returns_carry_dev == ret_stats_dev)) bad = "outputs must not be the same pointer as an input or as each other";
  if (int rc = bg_op_begin("bg_norm_reward_rows: ", bad, kernel_ms_out)) return rc;
  if (K == 0 || N == 0) return 0;
  const uint64_t chunks = bg_norm_rchunks(N);
  double* const part = (double*)workspace_dev;
  double* const mom_ws = part + (uint64_t)K * chunks * 2;
  double* const denom = mom_ws + (uint64_t)K * 2;
  double* const mom = moments_dev ? moments_dev : mom_ws;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (update) {
      hipLaunchKernelGGL(bg_norm_ret_partials, dim3((unsigned)chunks), dim3(BG_NORM_RBLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, (long long)chunks, gamma, returns_carry_dev, part);
      hipLaunchKernelGGL(bg_norm_ret_combine, dim3((unsigned)K), dim3(BG_NORM_RBLOCK), 0, s, part, (long long)N, (long long)chunks, mom);
      hipLaunchKernelGGL((bg_norm_ret_chain<true>), dim3(1), dim3(64), 0, s, mom, K, (double)N, epsilon, ret_stats_dev, denom);
    } else
      hipLaunchKernelGGL((bg_norm_ret_chain<false>), dim3(1), dim3(64), 0, s, mom, K, (double)N, epsilon, ret_stats_dev, denom);
    if (rewards_dev) {
      const long long m = (long long)K * (long long)N;
      hipLaunchKernelGGL(bg_norm_reward_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, rows_dev, row_stride_bytes, m, (long long)N, denom, update ? 1 : 0, clip_reward, rewards_dev);
    }
  });
}

// logits + action masks -> the policy head (bg_head.h).  The load paths follow the alignment of the caller's matrices.
// The load (or store) path of a logits-like [m, 60] matrix -- logits, their gradient, Q values -- from its alignment and its row pitch
static int bg_head_ld_path(const void* p, uint64_t stride, bool bf16) {
  const uint64_t es = bf16 ? 2u : 4u;
  const bool a16 = ((uintptr_t)p & 15) == 0;
  if (a16 && (stride * es) % 16 == 0) return BG_HEAD_LD_ROWS16;
  if (bf16 && a16 && stride == BG_HEAD_ACTIONS) return BG_HEAD_LD_FLAT16;
  if (!bf16 || (((uintptr_t)p & 3) == 0 && stride % 2 == 0)) return BG_HEAD_LD_WORD;
  return BG_HEAD_LD_HALF;
}
// The load path of the masks.  flat: the kernel reads the rows in order, so masks 60 bytes apart are one run (rows gathered through an index are not)
static int bg_head_mask_path(const int8_t* mask_dev, uint64_t mask_stride_bytes, bool flat) {
  if (!mask_dev) return BG_HEAD_LD_NONE;
  const bool m16 = ((uintptr_t)mask_dev & 15) == 0;
  return m16 && mask_stride_bytes % 16 == 0 ? BG_HEAD_LD_ROWS16 : flat && m16 && mask_stride_bytes == BG_HEAD_ACTIONS ? BG_HEAD_LD_FLAT16 : BG_HEAD_LD_WORD;
}
// The checks the head and the PPO loss share, in the order both make them: (dtype, m) first, the logits and the masks after the caller's own scalars
static const char* bg_head_shape_args(int logits_dtype, int64_t m) {
  if (logits_dtype != BG_HEAD_F32 && logits_dtype != BG_HEAD_BF16) return "logits_dtype must be BG_HEAD_F32 or BG_HEAD_BF16";
  if (m < 0 || m > (int64_t)BG_HEAD_ROWS * 0x7fffffffll) return "m out of range";
  return nullptr;
}
static const char* bg_head_logits_args(const void* logits_dev, uint64_t es, uint64_t logits_stride_elems) {
  if (!logits_dev || ((uintptr_t)logits_dev & (es - 1))) return "logits_dev must be a device pointer aligned to its element type";
  if (logits_stride_elems < BG_HEAD_ACTIONS || logits_stride_elems > 0xffffffffull) return "logits_stride_elems must be >= 60";
  return nullptr;
}
static const char* bg_head_mask_args(const int8_t* mask_dev, uint64_t mask_stride_bytes) {
  if (mask_dev && (((uintptr_t)mask_dev & 3) || mask_stride_bytes < BG_HEAD_ACTIONS || (mask_stride_bytes & 3) || mask_stride_bytes > 0xffffffffull)) return "mask_dev must be 4-byte aligned and mask_stride_bytes a multiple of 4, >= 60";
  return nullptr;
}

// What the head-ended calls (bg_head_call, bg_actor_head_call, bg_policy_forward) share behind their own inputs.  `act`: the call's one actions pointer,
// read by BG_HEAD_EVALUATE and written by the two drawing modes.
static const char* bg_head_out_args(const void* act, const float* log_prob_dev, const float* entropy_dev) {
  if (!act || ((uintptr_t)act & 3)) return "actions_dev must be a 4-byte aligned device pointer";
  if (((uintptr_t)log_prob_dev | (uintptr_t)entropy_dev) & 3) return "log_prob_dev / entropy_dev must be 4-byte aligned";
  return nullptr;
}
static int bg_head_mode(uint32_t flags, bool evaluate = false) { return evaluate ? BG_HEAD_EVALUATE : flags & BG_HEAD_DETERMINISTIC ? BG_HEAD_ARGMAX : BG_HEAD_SAMPLE; }
// logits_out (nullable, float32 [m, >= 60]) of the calls that compute their logits: its checks and its store path
static const char* bg_head_logits_out_args(const float* logits_out_dev, uint64_t logits_out_stride_elems) {
  if ((uintptr_t)logits_out_dev & 3) return "logits_out_dev must be 4-byte aligned";
  if (logits_out_dev && (logits_out_stride_elems < BG_HEAD_ACTIONS || logits_out_stride_elems > 0xffffffffull)) return "logits_out_stride_elems must be >= 60";
  return nullptr;
}
static int bg_head_logits_out_path(const float* p, uint64_t stride_elems) { return p ? bg_head_ld_path(p, stride_elems, false) : BG_HEAD_LD_WORD; }
// h (bfloat16 [m, width], read by 16-byte fragments) as verdicts: the refusal names the caller's own width, so its literal stays whole with the caller
static bool bg_head_bad_h(const void* h_dev) { return !h_dev || ((uintptr_t)h_dev & 15); }
static bool bg_head_bad_h_stride(uint64_t h_stride_elems, uint64_t width) { return h_stride_elems < width || (h_stride_elems & 7) || h_stride_elems > 0xffffffffull; }

static int bg_head_call(const char* who, int mode, const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev,
                        uint64_t mask_stride_bytes, int64_t m, uint64_t seed, uint64_t index0, uint64_t t, const int32_t* actions_in, int32_t* actions_out,
                        float* log_prob_dev, float* entropy_dev, float* kernel_ms_out, void* stream, float epsilon = 0.0f) {
  const bool bf16 = logits_dtype == BG_HEAD_BF16;
  const uint64_t es = bf16 ? 2u : 4u;
  const void* const act = mode == BG_HEAD_EVALUATE ? (const void*)actions_in : (const void*)actions_out;
  const void* const none[] = {nullptr};
  const void* const ins[] = {logits_dev, mask_dev};
  const void* const outs[] = {act, log_prob_dev, entropy_dev};   // (this call counts `act` among the outputs in every mode)
  const char* bad = bg_head_shape_args(logits_dtype, m);
  if (bad) {}
  else if (const char* r = bg_head_logits_args(logits_dev, es, logits_stride_elems)) bad = r;
  else if (const char* r = bg_head_mask_args(mask_dev, mask_stride_bytes)) bad = r;
  else if (const char* r = bg_head_out_args(act, log_prob_dev, entropy_dev)) bad = r;
  else if (bg_alias(none, outs)) bad = "actions_dev, log_prob_dev and entropy_dev must not be the same pointer";
  else if (bg_alias(ins, outs)) bad = "outputs must not alias the logits or the masks";
  if (int rc = bg_op_begin(who, bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const int lld = bg_head_ld_path(logits_dev, logits_stride_elems, bf16);
  const int mld = bg_head_mask_path(mask_dev, mask_stride_bytes, true);
  const unsigned grid = (unsigned)((m + BG_HEAD_ROWS - 1) / BG_HEAD_ROWS);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (mode == BG_HEAD_EPS) { hipLaunchKernelGGL(bg_head_eps_kernel, dim3(grid), dim3(BG_HEAD_BLOCK), 0, s, logits_dev, bf16 ? 1 : 0, lld, logits_stride_elems, mask_dev, mld, mask_stride_bytes, (long long)m, seed, index0, t, epsilon, actions_out); return; }
    bg_enc_pick<BG_HEAD_SAMPLE, BG_HEAD_ARGMAX, BG_HEAD_EVALUATE>(mode, [&](auto M) {
      hipLaunchKernelGGL((bg_head_kernel<M()>), dim3(grid), dim3(BG_HEAD_BLOCK), 0, s, logits_dev, bf16 ? 1 : 0, lld, logits_stride_elems, mask_dev, mld, mask_stride_bytes, (long long)m, seed, index0, t, actions_in, actions_out, log_prob_dev, entropy_dev);
    });
  });
}

int bg_sample_actions(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m,
                      uint32_t flags, uint64_t seed, uint64_t index0, uint64_t t, int32_t* actions_dev, float* log_prob_dev, float* entropy_dev,
                      float* kernel_ms_out, void* stream) {
  if (flags & ~BG_HEAD_DETERMINISTIC) { g_create_err = "bg_sample_actions: flags must be 0 or BG_HEAD_DETERMINISTIC"; return BG_E_ARG; }
  return bg_head_call("bg_sample_actions: ", bg_head_mode(flags), logits_dev, logits_dtype, logits_stride_elems, mask_dev,
                      mask_stride_bytes, m, seed, index0, t, nullptr, actions_dev, log_prob_dev, entropy_dev, kernel_ms_out, stream);
}
int bg_evaluate_actions(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m,
                        const int32_t* actions_dev, float* log_prob_dev, float* entropy_dev, float* kernel_ms_out, void* stream) {
  return bg_head_call("bg_evaluate_actions: ", BG_HEAD_EVALUATE, logits_dev, logits_dtype, logits_stride_elems, mask_dev, mask_stride_bytes, m, 0, 0, 0, actions_dev,
                      nullptr, log_prob_dev, entropy_dev, kernel_ms_out, stream);
}

// What the four loss calls (bg_ppo_loss, bg_bc_loss, bg_dqn_loss, bg_actor_ppo_loss) share.  The tests of the statistics, the workspace and a
// gradient matrix return a verdict only: the refusal names the caller's own constant or function, so its literal stays whole with the caller.
static bool bg_loss_bad_stats(const float* stats_dev) { return !stats_dev || ((uintptr_t)stats_dev & 3); }
static bool bg_loss_bad_workspace(int64_t m, const void* workspace_dev, uint64_t workspace_bytes, uint64_t need) {
  return m > 0 && (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < need);
}
static bool bg_loss_bad_matrix(const void* p, uint64_t es, uint64_t stride) { return !p || ((uintptr_t)p & (es - 1)) || stride < BG_HEAD_ACTIONS || stride > 0xffffffffull; }
static const char* bg_loss_dlogits_args(const void* dlogits_dev, uint64_t es, uint64_t dlogits_stride_elems) {
  if (!dlogits_dev || ((uintptr_t)dlogits_dev & (es - 1))) return "dlogits_dev must be a device pointer aligned to its element type";
  if (dlogits_stride_elems < BG_HEAD_ACTIONS || dlogits_stride_elems > 0xffffffffull) return "dlogits_stride_elems must be >= 60";
  return nullptr;
}
// m == 0: the statistics are zeros and nothing is launched
static int bg_loss_empty(float* stats_dev, int count, hipStream_t s) {
  BG_HIP0(hipMemsetAsync(stats_dev, 0, count * sizeof(float), s));
  return 0;
}

// logits + the stored arrays of a rollout -> PPO's loss, diagnostics and gradient (bg_ppo.h).  Workspace: BG_PPO_WS_HEAD bytes (mean, std, apply), one
// (n, mean, M2) triple per 256 rows, six float64 sums per 64 rows.
uint64_t bg_ppo_loss_workspace_bytes(int64_t m) { return m > 0 ? bg_ppo_ws_bytes(m) : 0; }

// What bg_ppo_loss and bg_actor_ppo_loss share beside the logits: the coefficients, and the stored arrays with the per-row outputs and the statistics.
// Each call makes the two checks around its own (the logits, or the layer), so every bad call gets the message it got.
struct BgPpoStored {
  const int8_t* mask_dev; uint64_t mask_stride_bytes;
  const int32_t* actions_dev; const float* old_log_prob_dev; const float* advantages_dev; const float* values_dev; const float* returns_dev;
  const int32_t* index_dev; int64_t store_rows;
  float* dvalues_dev; float* log_prob_dev; float* entropy_dev; float* stats_dev;
};
static const char* bg_ppo_coef_args(uint32_t flags, float clip_range, float ent_coef, float vf_coef) {
  if (flags & ~BG_PPO_NORMALIZE_ADV) return "flags must be 0 or BG_PPO_NORMALIZE_ADV";
  if (!(clip_range > 0.0f && clip_range < 1.0f)) return "clip_range must be in (0, 1)";
  if (!bg_ppo_finite(ent_coef) || !bg_ppo_finite(vf_coef)) return "ent_coef and vf_coef must be finite";
  return nullptr;
}
static const char* bg_ppo_stored_args(const BgPpoStored& S) {
  if (const char* r = bg_head_mask_args(S.mask_dev, S.mask_stride_bytes)) return r;
  if (!S.actions_dev || !S.old_log_prob_dev || !S.advantages_dev || (((uintptr_t)S.actions_dev | (uintptr_t)S.old_log_prob_dev | (uintptr_t)S.advantages_dev) & 3)) return "actions_dev, old_log_prob_dev and advantages_dev must be 4-byte aligned device pointers";
  if ((S.values_dev == nullptr) != (S.returns_dev == nullptr)) return "values_dev and returns_dev go together: both or neither";
  if (((uintptr_t)S.values_dev | (uintptr_t)S.returns_dev | (uintptr_t)S.index_dev | (uintptr_t)S.dvalues_dev | (uintptr_t)S.log_prob_dev | (uintptr_t)S.entropy_dev) & 3) return "values_dev, returns_dev, index_dev, dvalues_dev, log_prob_dev and entropy_dev must be 4-byte aligned";
  if (S.dvalues_dev && !S.values_dev) return "dvalues_dev needs values_dev and returns_dev";
  if (S.index_dev && (S.store_rows < 0 || S.store_rows > 0x7fffffffll)) return "store_rows must be in [0, 2**31) when index_dev is given";
  if (bg_loss_bad_stats(S.stats_dev)) return "stats_dev must be a 4-byte aligned device pointer to BG_PPO_STATS floats";
  return nullptr;
}
// The kernels' arguments, but for the logits and their gradient (lld, dst and the four fields of the two matrices: the caller's), with the workspace
// carved up: head, statistics partials, row partials.
static BgPpoArgs bg_ppo_args(const BgPpoStored& S, int64_t m, float clip_range, float ent_coef, float vf_coef, uint32_t flags, void* workspace_dev) {
  BgPpoArgs A;
  A.mask = S.mask_dev; A.mstride = S.mask_stride_bytes; A.mld = bg_head_mask_path(S.mask_dev, S.mask_stride_bytes, !S.index_dev);
  A.actions = S.actions_dev; A.old_lp = S.old_log_prob_dev; A.adv = S.advantages_dev; A.values = S.values_dev; A.returns = S.returns_dev;
  A.index = S.index_dev; A.store_rows = (long long)S.store_rows; A.m = (long long)m;
  A.c.clip = clip_range; A.c.lo = 1.0f - clip_range; A.c.hi = 1.0f + clip_range; A.c.ent_coef = ent_coef; A.c.vf_coef = vf_coef; A.c.fm = (float)m;
  A.normalize = flags & BG_PPO_NORMALIZE_ADV ? 1 : 0;
  A.dvalues = S.dvalues_dev; A.log_prob = S.log_prob_dev; A.entropy = S.entropy_dev;
  A.head = (const float*)workspace_dev;
  A.partials = (double*)((BgPpoMoments*)((uint8_t*)workspace_dev + BG_PPO_WS_HEAD) + bg_ppo_stat_parts(m));
  return A;
}
// the launches in front of and behind the row pass: the advantage statistics (with BG_PPO_NORMALIZE_ADV), and the finish
static void bg_ppo_launch_adv(const BgPpoArgs& A, hipStream_t s) {
  if (!A.normalize) return;
  float* const head = (float*)A.head;
  BgPpoMoments* const mom = (BgPpoMoments*)((uint8_t*)head + BG_PPO_WS_HEAD);
  const uint64_t SP = bg_ppo_stat_parts(A.m);
  hipLaunchKernelGGL(bg_ppo_adv_partials, dim3((unsigned)SP), dim3(BG_PPO_LANES), 0, s, A.adv, A.index, A.store_rows, A.m, mom);
  hipLaunchKernelGGL(bg_ppo_adv_combine, dim3(1), dim3(BG_PPO_LANES), 0, s, mom, (long long)SP, head);
}
static void bg_ppo_launch_finish(const BgPpoArgs& A, float* stats_dev, hipStream_t s) {
  hipLaunchKernelGGL(bg_ppo_finish, dim3(1), dim3(BG_PPO_LANES), 0, s, A.partials, (long long)bg_ppo_row_parts(A.m), A.m, A.c.ent_coef, A.c.vf_coef, A.normalize, A.head, stats_dev);
}

int bg_ppo_loss(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes,
                const int32_t* actions_dev, const float* old_log_prob_dev, const float* advantages_dev, const float* values_dev, const float* returns_dev,
                const int32_t* index_dev, int64_t store_rows, int64_t m, float clip_range, float ent_coef, float vf_coef, uint32_t flags, void* dlogits_dev,
                uint64_t dlogits_stride_elems, float* dvalues_dev, float* log_prob_dev, float* entropy_dev, float* stats_dev, void* workspace_dev,
                uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const bool bf16 = logits_dtype == BG_HEAD_BF16;
  const uint64_t es = bf16 ? 2u : 4u;
  const void* const ins[] = {logits_dev, mask_dev, actions_dev, old_log_prob_dev, advantages_dev, values_dev, returns_dev, index_dev};
  const void* const outs[] = {dlogits_dev, dvalues_dev, log_prob_dev, entropy_dev, stats_dev, workspace_dev};
  const BgPpoStored S = {mask_dev, mask_stride_bytes, actions_dev, old_log_prob_dev, advantages_dev, values_dev, returns_dev, index_dev, store_rows,
                         dvalues_dev, log_prob_dev, entropy_dev, stats_dev};
  const char* bad = bg_head_shape_args(logits_dtype, m);
  if (bad) {}
  else if (const char* r = bg_ppo_coef_args(flags, clip_range, ent_coef, vf_coef)) bad = r;
  else if (const char* r = bg_head_logits_args(logits_dev, es, logits_stride_elems)) bad = r;
  else if (const char* r = bg_loss_dlogits_args(dlogits_dev, es, dlogits_stride_elems)) bad = r;
  else if (const char* r = bg_ppo_stored_args(S)) bad = r;
  else if (bg_loss_bad_workspace(m, workspace_dev, workspace_bytes, bg_ppo_loss_workspace_bytes(m))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_ppo_loss_workspace_bytes(m) bytes";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_ppo_loss: ", bad, kernel_ms_out)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return bg_loss_empty(stats_dev, BG_PPO_STATS, s);
  BgPpoArgs A = bg_ppo_args(S, m, clip_range, ent_coef, vf_coef, flags, workspace_dev);
  A.logits = logits_dev; A.lstride = logits_stride_elems; A.lld = bg_head_ld_path(logits_dev, logits_stride_elems, bf16);
  A.dlogits = dlogits_dev; A.dstride = dlogits_stride_elems; A.dst = bg_head_ld_path(dlogits_dev, dlogits_stride_elems, bf16);
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_ppo_launch_adv(A, s);
    bg_bool_dispatch(bf16, false, [&](auto BF16, auto) {
      hipLaunchKernelGGL((bg_ppo_kernel<BF16()>), dim3((unsigned)bg_ppo_row_parts(m)), dim3(BG_HEAD_BLOCK), 0, s, A);
    });
    bg_ppo_launch_finish(A, stats_dev, s);
  });
}

// epsilon-greedy over the masked head (bg_dqn.h): bg_sample_actions' arguments and checks, plus epsilon; no log_prob / entropy
int bg_sample_actions_eps(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m,
                          uint32_t flags, uint64_t seed, uint64_t index0, uint64_t t, float epsilon, int32_t* actions_dev, float* log_prob_dev,
                          float* entropy_dev, float* kernel_ms_out, void* stream) {
  if (flags) { g_create_err = "bg_sample_actions_eps: flags must be 0"; return BG_E_ARG; }
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) { g_create_err = "bg_sample_actions_eps: epsilon must be in [0, 1]"; return BG_E_ARG; }
  if (log_prob_dev || entropy_dev) { g_create_err = "bg_sample_actions_eps: log_prob_dev and entropy_dev must be NULL (an epsilon-greedy action has no categorical log-probability)"; return BG_E_ARG; }
  return bg_head_call("bg_sample_actions_eps: ", BG_HEAD_EPS, logits_dev, logits_dtype, logits_stride_elems, mask_dev, mask_stride_bytes, m, seed, index0, t, nullptr,
                      actions_dev, nullptr, nullptr, kernel_ms_out, stream, epsilon);
}

// packed records -> the outcome of every step's own episode (bg_outcome.h): one scan backwards along K, bg_gae_rows' shape
int bg_episode_outcome_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, double gamma, const double* rewards_dev,
                            const int32_t* tail_steps_dev, const int32_t* tail_ante_dev, const uint8_t* tail_flags_dev, const double* tail_return_dev,
                            int32_t* steps_to_end_dev, int32_t* end_ante_dev, uint8_t* end_flags_dev, double* returns_dev, float* kernel_ms_out, void* stream) {
  const void* const ins[] = {rows_dev, rewards_dev, tail_steps_dev, tail_ante_dev, tail_flags_dev, tail_return_dev};
  const void* const outs[] = {steps_to_end_dev, end_ante_dev, end_flags_dev, returns_dev};
  const char* bad = bg_scan_args(rows_dev, row_stride_bytes, K, N);
  if (bad) {}
  else if (!steps_to_end_dev && !end_ante_dev && !end_flags_dev && !returns_dev) bad = "at least one of steps_to_end_dev, end_ante_dev, end_flags_dev and returns_dev must be given";
  else if ((tail_steps_dev && !steps_to_end_dev) || (tail_ante_dev && !end_ante_dev) || (tail_flags_dev && !end_flags_dev) || (tail_return_dev && !returns_dev)) bad = "a tail needs its output";
  else if (rewards_dev && !returns_dev) bad = "rewards_dev needs returns_dev (no other output reads a reward)";
  else if (!(gamma == gamma)) bad = "gamma must not be NaN";
  else if (((uintptr_t)steps_to_end_dev | (uintptr_t)end_ante_dev | (uintptr_t)tail_steps_dev | (uintptr_t)tail_ante_dev) & 3) bad = "int32 arrays must be 4-byte aligned";
  else if (((uintptr_t)returns_dev | (uintptr_t)rewards_dev | (uintptr_t)tail_return_dev) & 7) bad = "float64 arrays must be 8-byte aligned";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_episode_outcome_rows: ", bad, kernel_ms_out)) return rc;
  if (K == 0 || N == 0) return 0;
  const unsigned grid = (unsigned)((N + BG_GAE_ENVS - 1) / BG_GAE_ENVS);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_bool_dispatch(returns_dev != nullptr, returns_dev != nullptr && rewards_dev != nullptr, [&](auto R, auto W) {
      hipLaunchKernelGGL((bg_outcome_kernel<R(), R() && W()>), dim3(grid), dim3(BG_GAE_BLOCK), 0, s, rows_dev, row_stride_bytes, K, (long long)N, gamma, rewards_dev,
                         tail_steps_dev, tail_ante_dev, tail_flags_dev, tail_return_dev, steps_to_end_dev, end_ante_dev, end_flags_dev, returns_dev);
    });
  });
}

// logits + stored actions -> behaviour cloning's weighted cross-entropy, its accuracy and its gradient (bg_bc.h).  Workspace: BG_BC_WS_HEAD bytes
// (Wf, W), one float64 weight sum per 256 rows, four float64 sums per 64 rows.
uint64_t bg_bc_loss_workspace_bytes(int64_t m) {
  if (m <= 0) return 0;
  return BG_BC_WS_HEAD + bg_ppo_stat_parts(m) * sizeof(double) + bg_ppo_row_parts(m) * (BG_BC_SUMS * sizeof(double));
}

int bg_bc_loss(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes,
               const int32_t* actions_dev, uint64_t actions_stride_bytes, const float* weights_dev, const int32_t* index_dev, int64_t store_rows, int64_t m,
               float ent_coef, void* dlogits_dev, uint64_t dlogits_stride_elems, float* log_prob_dev, float* entropy_dev, float* stats_dev,
               void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const bool bf16 = logits_dtype == BG_HEAD_BF16;
  const uint64_t es = bf16 ? 2u : 4u;
  const void* const ins[] = {logits_dev, mask_dev, actions_dev, weights_dev, index_dev};
  const void* const outs[] = {dlogits_dev, log_prob_dev, entropy_dev, stats_dev, workspace_dev};
  const char* bad = bg_head_shape_args(logits_dtype, m);
  if (bad) {}
  else if (!bg_ppo_finite(ent_coef)) bad = "ent_coef must be finite";
  else if (const char* r = bg_head_logits_args(logits_dev, es, logits_stride_elems)) bad = r;
  else if (const char* r = bg_loss_dlogits_args(dlogits_dev, es, dlogits_stride_elems)) bad = r;
  else if (const char* r = bg_head_mask_args(mask_dev, mask_stride_bytes)) bad = r;
  else if (!actions_dev || ((uintptr_t)actions_dev & 3)) bad = "actions_dev must be a 4-byte aligned device pointer";
  else if (actions_stride_bytes < 4 || (actions_stride_bytes & 3) || actions_stride_bytes > 0xffffffffull) bad = "actions_stride_bytes must be a multiple of 4, >= 4";
  else if (((uintptr_t)weights_dev | (uintptr_t)index_dev | (uintptr_t)log_prob_dev | (uintptr_t)entropy_dev) & 3) bad = "weights_dev, index_dev, log_prob_dev and entropy_dev must be 4-byte aligned";
  else if (index_dev && (store_rows < 0 || store_rows > 0x7fffffffll)) bad = "store_rows must be in [0, 2**31) when index_dev is given";
  else if (bg_loss_bad_stats(stats_dev)) bad = "stats_dev must be a 4-byte aligned device pointer to BG_BC_STATS floats";
  else if (bg_loss_bad_workspace(m, workspace_dev, workspace_bytes, bg_bc_loss_workspace_bytes(m))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_bc_loss_workspace_bytes(m) bytes";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_bc_loss: ", bad, kernel_ms_out)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return bg_loss_empty(stats_dev, BG_BC_STATS, s);
  const bool stat = weights_dev || index_dev;
  BgBcArgs A;
  A.logits = logits_dev; A.lstride = logits_stride_elems; A.lld = bg_head_ld_path(logits_dev, logits_stride_elems, bf16);
  A.dst = bg_head_ld_path(dlogits_dev, dlogits_stride_elems, bf16);
  A.mask = mask_dev; A.mstride = mask_stride_bytes; A.mld = bg_head_mask_path(mask_dev, mask_stride_bytes, !index_dev);
  A.actions = actions_dev; A.astride = actions_stride_bytes; A.weights = weights_dev;
  A.index = index_dev; A.store_rows = (long long)store_rows; A.m = (long long)m;
  A.ent_coef = ent_coef; A.fm = (float)m;
  A.dlogits = dlogits_dev; A.dstride = dlogits_stride_elems; A.log_prob = log_prob_dev; A.entropy = entropy_dev;
  float* const head = (float*)workspace_dev;
  double* const wpart = (double*)((uint8_t*)workspace_dev + BG_BC_WS_HEAD);
  const uint64_t SP = bg_ppo_stat_parts(m), RP = bg_ppo_row_parts(m);
  A.head = stat ? head : nullptr; A.partials = wpart + SP;
  return bg_op_run(kernel_ms_out, s, [&] {
    if (stat) {
      hipLaunchKernelGGL(bg_bc_weight_partials, dim3((unsigned)SP), dim3(BG_PPO_LANES), 0, s, weights_dev, index_dev, (long long)store_rows, (long long)m, wpart);
      hipLaunchKernelGGL(bg_bc_weight_combine, dim3(1), dim3(BG_PPO_LANES), 0, s, wpart, (long long)SP, head);
    }
    bg_bool_dispatch(bf16, false, [&](auto BF16, auto) {
      hipLaunchKernelGGL((bg_bc_kernel<BF16()>), dim3((unsigned)RP), dim3(BG_HEAD_BLOCK), 0, s, A);
    });
    hipLaunchKernelGGL(bg_bc_finish, dim3(1), dim3(BG_PPO_LANES), 0, s, A.partials, (long long)RP, (long long)m, ent_coef, A.head, stats_dev);
  });
}

// Q values + the ring of records -> DQN's TD loss, diagnostics and gradient (bg_dqn.h).  Workspace: seven float64 values per 64 rows.
uint64_t bg_dqn_loss_workspace_bytes(int64_t m) {
  if (m <= 0) return 0;
  return bg_dqn_row_parts(m) * (BG_DQN_SUMS * sizeof(double));
}

int bg_dqn_loss(const void* q_dev, uint64_t q_stride_elems, const void* q_next_dev, uint64_t q_next_stride_elems, const void* q_next_online_dev,
                uint64_t q_next_online_stride_elems, int q_dtype, const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                const int32_t* next_index_dev, const float* rewards_dev, int64_t m, float gamma, uint32_t flags, void* dq_dev, uint64_t dq_stride_elems,
                float* td_dev, float* stats_dev, void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const bool bf16 = q_dtype == BG_HEAD_BF16;
  const uint64_t es = bf16 ? 2u : 4u;
  const void* const ins[] = {q_dev, q_next_dev, q_next_online_dev, rows_dev, next_index_dev, rewards_dev};
  const void* const outs[] = {dq_dev, td_dev, stats_dev, workspace_dev};
  const char* bad = nullptr;
  if (q_dtype != BG_HEAD_F32 && q_dtype != BG_HEAD_BF16) bad = "q_dtype must be BG_HEAD_F32 or BG_HEAD_BF16";
  else if (m < 0 || m > (int64_t)BG_HEAD_ROWS * 0x7fffffffll) bad = "m out of range";
  else if (flags & ~(BG_DQN_MASK_NEXT | BG_DQN_MSE | BG_DQN_TIMEOUT_EXCLUDE)) bad = "flags must be a combination of BG_DQN_MASK_NEXT, BG_DQN_MSE and BG_DQN_TIMEOUT_EXCLUDE";
  else if (!(gamma >= 0.0f && gamma <= 1.0f)) bad = "gamma must be in [0, 1]";
  else if (bg_loss_bad_matrix(q_dev, es, q_stride_elems)) bad = "q_dev must be a device pointer aligned to its element type, q_stride_elems >= 60";
  else if (bg_loss_bad_matrix(q_next_dev, es, q_next_stride_elems)) bad = "q_next_dev must be a device pointer aligned to its element type, q_next_stride_elems >= 60";
  else if (q_next_online_dev && bg_loss_bad_matrix(q_next_online_dev, es, q_next_online_stride_elems)) bad = "q_next_online_dev must be aligned to its element type, q_next_online_stride_elems >= 60";
  else if (bg_loss_bad_matrix(dq_dev, es, dq_stride_elems)) bad = "dq_dev must be a device pointer aligned to its element type, dq_stride_elems >= 60";
  else if (!rows_dev || ((uintptr_t)rows_dev & 15)) bad = "rows_dev must be a 16-byte aligned device pointer";
  else if (row_stride_bytes < BG_ROW_BYTES || (row_stride_bytes & 15) || row_stride_bytes > 0xffffffffull) bad = "row_stride_bytes must be a multiple of 16, >= BG_ROW_BYTES";
  else if (store_rows < 0 || store_rows > 0x7fffffffll) bad = "store_rows must be in [0, 2**31)";
  else if (!next_index_dev || ((uintptr_t)next_index_dev & 3)) bad = "next_index_dev must be a 4-byte aligned device pointer";
  else if (((uintptr_t)rewards_dev | (uintptr_t)td_dev) & 3) bad = "rewards_dev and td_dev must be 4-byte aligned";
  else if (bg_loss_bad_stats(stats_dev)) bad = "stats_dev must be a 4-byte aligned device pointer to BG_DQN_STATS floats";
  else if (bg_loss_bad_workspace(m, workspace_dev, workspace_bytes, bg_dqn_loss_workspace_bytes(m))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_dqn_loss_workspace_bytes(m) bytes";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_dqn_loss: ", bad, kernel_ms_out)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return bg_loss_empty(stats_dev, BG_DQN_STATS, s);
  BgDqnArgs A;
  A.q = q_dev; A.qstride = q_stride_elems;
  A.qn = q_next_dev; A.nstride = q_next_stride_elems; A.nld = bg_head_ld_path(q_next_dev, q_next_stride_elems, bf16);
  A.qo = q_next_online_dev; A.ostride = q_next_online_stride_elems; A.old = q_next_online_dev ? bg_head_ld_path(q_next_online_dev, q_next_online_stride_elems, bf16) : BG_HEAD_LD_NONE;
  A.rows = rows_dev; A.rstride = row_stride_bytes; A.store_rows = (long long)store_rows;
  A.next_index = next_index_dev; A.rewards = rewards_dev; A.m = (long long)m;
  A.gamma = gamma; A.fm = (float)m; A.flags = flags;
  A.dq = dq_dev; A.dstride = dq_stride_elems; A.dst = bg_head_ld_path(dq_dev, dq_stride_elems, bf16);
  A.td = td_dev; A.partials = (double*)workspace_dev;
  const uint64_t RP = bg_dqn_row_parts(m);
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_bool_dispatch(q_next_online_dev != nullptr, bf16, [&](auto DOUBLE, auto BF16) {
      hipLaunchKernelGGL((bg_dqn_kernel<BF16(), DOUBLE()>), dim3((unsigned)RP), dim3(BG_HEAD_BLOCK), 0, s, A);
    });
    hipLaunchKernelGGL(bg_dqn_finish, dim3(1), dim3(BG_DQN_LANES), 0, s, A.partials, (long long)RP, (long long)m, stats_dev);
  });
}

// packed records -> a network's first layer and its weight / bias gradient: bg_linear_rows (bg_linear.h: the features of bg_encode_rows_ex are built
// in LDS and consumed by the matrix cores in the same launch) and, at the end of this header, bg_extractor_rows (bg_extractor.h).  The two families make
// the same checks in the same order; a BgFirstLayer states what differs: the weight's columns, the three refusals that name them or the workspace
// function, and that function.
struct BgFirstLayer {
  int K;
  const char *bad_weight_stride, *bad_dweight_stride, *bad_workspace;
  uint64_t (*workspace_bytes)(int64_t m, int H);
};
static const BgFirstLayer bg_linear_layer = {BG_LIN_K, "weight_stride_elems must be in [153, 2**24]", "dweight_stride_elems must be >= 153",
                                             "workspace_dev must be a 16-byte aligned device buffer of bg_linear_rows_workspace_bytes(m, H) bytes",
                                             bg_linear_rows_workspace_bytes};

// what all four entry points check of the layer's shape, the records and the index
static const char* bg_first_common_args(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, int H,
                                        int activation) {
  if (H < 32 || H > 4096 || H % 32) return "H must be a multiple of 32 in [32, 4096]";
  if (activation != BG_LIN_NONE && activation != BG_LIN_RELU) return "activation must be BG_LIN_NONE or BG_LIN_RELU";
  if (m < 0 || m > (int64_t)BG_LIN_ROWS * 0x7fffffffll) return "m out of range";
  if (store_rows < 0) return "store_rows must be >= 0";
  if (index_dev && store_rows > 0x7fffffffll) return "store_rows must be in [0, 2**31) when index_dev is given";
  if (!index_dev && m > store_rows) return "m must be <= store_rows when index_dev is NULL";
  if (const char* r = bg_rows_args(rows_dev, row_stride_bytes)) return r;
  if ((uintptr_t)index_dev & 3) return "index_dev must be 4-byte aligned";
  return nullptr;
}
// ... with the layout in front of it and the statistics behind it: the linear calls
static const char* bg_linear_common_args(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, int layout,
                                         const double* mean_dev, const double* var_dev, double epsilon, double clip_obs, int H, int activation) {
  const bool norm = mean_dev || var_dev;
  if (layout == BG_ENC_EXTRACTOR) return "layout BG_ENC_EXTRACTOR is not supported (its 416 one-hot columns want an embedding gather): BG_ENC_PRODUCED or BG_ENC_FIXED";
  if (layout != BG_ENC_PRODUCED && layout != BG_ENC_FIXED) return "layout must be BG_ENC_PRODUCED or BG_ENC_FIXED";
  if (const char* r = bg_first_common_args(rows_dev, row_stride_bytes, store_rows, index_dev, m, H, activation)) return r;
  if (norm && (!mean_dev || !var_dev)) return "mean_dev and var_dev go together: both or neither";
  if (norm && (((uintptr_t)mean_dev | (uintptr_t)var_dev) & 7)) return "mean_dev and var_dev must be 8-byte aligned";
  if (norm && mean_dev == var_dev) return "mean_dev and var_dev must not be the same pointer";
  if (norm && !(epsilon >= 0.0 && epsilon <= 1.7976931348623157e308 && clip_obs >= 0.0 && clip_obs <= 1.7976931348623157e308)) return "epsilon and clip_obs must be finite and >= 0 when statistics are given";
  return nullptr;
}
// the forward's weight, bias and out; out must be none of the inputs (mean_dev / var_dev: NULL where the call has no statistics)
static const char* bg_first_forward_args(const BgFirstLayer& L, const uint8_t* rows_dev, const int32_t* index_dev, const double* mean_dev, const double* var_dev,
                                         const void* weight_dev, uint64_t weight_stride_elems, const float* bias_dev, int H, int out_dtype, void* out_dev,
                                         uint64_t out_stride_elems) {
  const uint64_t es = out_dtype == BG_ENC_F32 ? 4u : 2u;
  if (out_dtype != BG_ENC_F32 && out_dtype != BG_ENC_BF16) return "out_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  if (!weight_dev || ((uintptr_t)weight_dev & 1)) return "weight_dev must be a 2-byte aligned device pointer";
  if (weight_stride_elems < (uint64_t)L.K || weight_stride_elems > 0x1000000ull) return L.bad_weight_stride;
  if ((uintptr_t)bias_dev & 3) return "bias_dev must be 4-byte aligned";
  if (!out_dev || ((uintptr_t)out_dev & (es - 1))) return "out_dev must be a device pointer aligned to its element type";
  if (out_stride_elems < (uint64_t)H || out_stride_elems > 0xffffffffull) return "out_stride_elems must be >= H";
  if (out_dev == (const void*)rows_dev || out_dev == (const void*)index_dev || out_dev == (const void*)mean_dev || out_dev == (const void*)var_dev ||
      out_dev == weight_dev || out_dev == (const void*)bias_dev) return "out_dev must not be the same pointer as an input";
  return nullptr;
}
// the gradient's dout, out, dweight, dbias and workspace, and that no output or workspace is an input or another output
static const char* bg_first_grad_args(const BgFirstLayer& L, const uint8_t* rows_dev, int64_t m, const void* dout_dev, int dout_dtype, uint64_t dout_stride_elems,
                                      const void* out_dev, int out_dtype, uint64_t out_stride_elems, int H, int activation, float* dweight_dev,
                                      uint64_t dweight_stride_elems, float* dbias_dev, void* workspace_dev, uint64_t workspace_bytes) {
  const uint64_t ds = dout_dtype == BG_ENC_F32 ? 4u : 2u, os = out_dtype == BG_ENC_F32 ? 4u : 2u;
  const bool relu = activation == BG_LIN_RELU;
  if (dout_dtype != BG_ENC_F32 && dout_dtype != BG_ENC_BF16) return "dout_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  if (!dout_dev || ((uintptr_t)dout_dev & (ds - 1))) return "dout_dev must be a device pointer aligned to its element type";
  if (dout_stride_elems < (uint64_t)H || dout_stride_elems > 0xffffffffull) return "dout_stride_elems must be >= H";
  if (relu != (out_dev != nullptr)) return "out_dev (the forward's output) is required with BG_LIN_RELU and must be NULL without it";
  if (relu && out_dtype != BG_ENC_F32 && out_dtype != BG_ENC_BF16) return "out_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  if (relu && (((uintptr_t)out_dev & (os - 1)) || out_stride_elems < (uint64_t)H || out_stride_elems > 0xffffffffull)) return "out_dev must be aligned to its element type and out_stride_elems >= H";
  if (!dweight_dev || (((uintptr_t)dweight_dev | (uintptr_t)dbias_dev) & 3)) return "dweight_dev must be a 4-byte aligned device pointer (dbias_dev 4-byte aligned)";
  if (dweight_stride_elems < (uint64_t)L.K || dweight_stride_elems > 0xffffffffull) return L.bad_dweight_stride;
  if (m > 0 && (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < L.workspace_bytes(m, H))) return L.bad_workspace;
  if ((const void*)dweight_dev == dout_dev || (const void*)dweight_dev == out_dev || (const void*)dweight_dev == (const void*)rows_dev || dweight_dev == dbias_dev ||
      (void*)dweight_dev == workspace_dev || (dbias_dev && ((void*)dbias_dev == workspace_dev || (const void*)dbias_dev == dout_dev || (const void*)dbias_dev == out_dev)) ||
      workspace_dev == dout_dev || (workspace_dev && workspace_dev == out_dev)) return "outputs and the workspace must not be the same pointer as an input or as each other";
  return nullptr;
}
// the forward's grid.y: a short call spreads the chunks of H over more workgroups (a function of m and H alone)
static unsigned bg_first_ysplit(unsigned gx, int H) {
  const unsigned nchunks = (unsigned)((H + BG_LIN_WCHUNK - 1) / BG_LIN_WCHUNK);
  unsigned ys = 1;
  while ((uint64_t)gx * ys < 512u && ys * 2u <= nchunks) ys *= 2u;
  return ys;
}

int bg_linear_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, int layout,
                   const double* mean_dev, const double* var_dev, double epsilon, double clip_obs, const void* weight_dev, uint64_t weight_stride_elems,
                   const float* bias_dev, int H, int activation, int out_dtype, void* out_dev, uint64_t out_stride_elems, float* kernel_ms_out, void* stream) {
  const char* bad = bg_linear_common_args(rows_dev, row_stride_bytes, store_rows, index_dev, m, layout, mean_dev, var_dev, epsilon, clip_obs, H, activation);
  if (!bad) bad = bg_first_forward_args(bg_linear_layer, rows_dev, index_dev, mean_dev, var_dev, weight_dev, weight_stride_elems, bias_dev, H, out_dtype, out_dev, out_stride_elems);
  if (int rc = bg_op_begin("bg_linear_rows: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const unsigned gx = (unsigned)bg_lin_blocks(m), ys = bg_first_ysplit(gx, H);
  hipStream_t s = (hipStream_t)stream;
  const int relu = activation == BG_LIN_RELU;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_bool_dispatch(mean_dev != nullptr, out_dtype == BG_ENC_F32, [&](auto NORM, auto F32) {
      hipLaunchKernelGGL((bg_linear_rows_kernel<NORM(), F32() ? BG_ENC_F32 : BG_ENC_BF16>), dim3(gx, ys), dim3(BG_LIN_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, mean_dev, var_dev, epsilon, clip_obs, (const uint16_t*)weight_dev, weight_stride_elems, bias_dev, H, relu, out_dev, out_stride_elems);
    });
  });
}

uint64_t bg_linear_rows_workspace_bytes(int64_t m, int H) { return bg_lin_workspace_bytes(m, H, 1, BG_LIN_PART_ROWS); }

int bg_linear_rows_grad(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, int layout,
                        const double* mean_dev, const double* var_dev, double epsilon, double clip_obs, const void* dout_dev, int dout_dtype,
                        uint64_t dout_stride_elems, const void* out_dev, int out_dtype, uint64_t out_stride_elems, int H, int activation,
                        float* dweight_dev, uint64_t dweight_stride_elems, float* dbias_dev, void* workspace_dev, uint64_t workspace_bytes,
                        float* kernel_ms_out, void* stream) {
  const char* bad = bg_linear_common_args(rows_dev, row_stride_bytes, store_rows, index_dev, m, layout, mean_dev, var_dev, epsilon, clip_obs, H, activation);
  if (!bad) bad = bg_first_grad_args(bg_linear_layer, rows_dev, m, dout_dev, dout_dtype, dout_stride_elems, out_dev, out_dtype, out_stride_elems, H, activation, dweight_dev, dweight_stride_elems, dbias_dev, workspace_dev, workspace_bytes);
  if (int rc = bg_op_begin("bg_linear_rows_grad: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const long long per = bg_lin_blocks_per_group(m, H), groups = bg_lin_groups(m, H);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    auto go = [&](auto NORM) {
      hipLaunchKernelGGL((bg_linear_rows_grad_kernel<NORM()>), dim3((unsigned)groups, (unsigned)bg_lin_spans(H)), dim3(BG_LIN_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, mean_dev, var_dev, epsilon, clip_obs, dout_dev, (int)(dout_dtype == BG_ENC_BF16), dout_stride_elems, out_dev, (int)(out_dtype == BG_ENC_BF16), out_stride_elems, H, per, (float*)workspace_dev);
    };
    if (mean_dev) go(std::true_type{}); else go(std::false_type{});
    const long long items = (long long)BG_LIN_PART_ROWS * H;
    hipLaunchKernelGGL(bg_linear_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const float*)workspace_dev, groups, H, dweight_dev, dweight_stride_elems, dbias_dev);
  });
}

static int bg_batch_dev(BgDev& d, int m, uint32_t** scratch_out);

int bg_score_hand_batch_ex(const int32_t* cases_dev, int64_t* out_dev, int m, int lanes_per_case, float* kernel_ms_out, void* stream) {
  if (!cases_dev || !out_dev || m < 0 || (lanes_per_case != 1 && lanes_per_case != 8)) { g_create_err = "bg_score_hand_batch: bad arguments (lanes_per_case 1 or 8)"; return BG_E_ARG; }
  if (kernel_ms_out) *kernel_ms_out = 0.f;
  if (m == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  BgDev d;
  uint32_t* scratch = nullptr; // two MT19937 blocks per case + the error word
  int rc = bg_batch_dev(d, m, &scratch);
  if (rc) return rc;
  BgOpTimer tm;
  hipError_t e = hipMemsetAsync(d.err, 0, 4 * sizeof(uint32_t), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bg_score_seed_kernel, dim3((m + BG_BLOCK - 1) / BG_BLOCK), dim3(BG_BLOCK), 0, s, d, cases_dev); // random.seed(gseed) per case
    rc = tm.begin(kernel_ms_out, s);
    if (lanes_per_case == 1)
      hipLaunchKernelGGL(bg_score_hand_batch_kernel, dim3((m + BG_BLOCK - 1) / BG_BLOCK), dim3(BG_BLOCK), 0, s, d, cases_dev, out_dev);
    else
      hipLaunchKernelGGL(bg_score_hand_batch_l8_kernel, dim3((m + BG_BLOCK / 8 - 1) / (BG_BLOCK / 8)), dim3(BG_BLOCK), 0, s, d, cases_dev, out_dev);
    tm.mark(s);
    e = hipGetLastError();
  }
  uint32_t errw = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&errw, d.err, sizeof(errw), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && rc == 0) rc = tm.end(kernel_ms_out);
  (void)hipFree(scratch);
  if (e != hipSuccess) { g_create_err = std::string("bg_score_hand_batch: ") + hipGetErrorString(e); return BG_E_HIP; }
  if (rc) return rc;
  if (errw) { g_create_err = "bg_score_hand_batch: a case drew more than two blocks of the global stream"; return BG_E_INTERNAL; }
  return 0;
}
int bg_score_hand_batch(const int32_t* cases_dev, int64_t* out_dev, int m, void* stream) {
  return bg_score_hand_batch_ex(cases_dev, out_dev, m, 1, nullptr, stream);
}

// scratch of a batch op that draws from a per-case global stream: two MT19937 blocks per case + the device error word
static int bg_batch_dev(BgDev& d, int m, uint32_t** scratch_out) {
  memset(&d, 0, sizeof(d));
  d.N = m; d.flags = BG_FLAG_SCORER_JOKERS; d.KG = 2; d.KS = 2; d.KD = 1;
  uint32_t* scratch = nullptr;
  BG_HIP0(hipMalloc((void**)&scratch, ((size_t)m * 2 * BG_MTS + 4) * sizeof(uint32_t)));
  d.gblk = scratch; d.err = scratch + (size_t)m * 2 * BG_MTS;
  *scratch_out = scratch;
  return 0;
}

int bg_sim_evaluate_batch(const int32_t* hands_dev, const int32_t* n_dev, const int32_t* flags_dev, int8_t* out_dev, int m, void* stream) {
  if (!hands_dev || !n_dev || !flags_dev || !out_dev || m < 0) { g_create_err = "bg_sim_evaluate_batch: bad arguments"; return BG_E_ARG; }
  if (m == 0) return 0;
  hipLaunchKernelGGL(bg_sim_evaluate_batch_kernel, dim3((m + BG_BLOCK - 1) / BG_BLOCK), dim3(BG_BLOCK), 0, (hipStream_t)stream, hands_dev, n_dev, flags_dev, out_dev, m);
  BG_HIP0(hipGetLastError());
  return 0;
}

int bg_sim_score_batch(const int32_t* cases_dev, int64_t* out_dev, int m, void* stream) {
  if (!cases_dev || !out_dev || m < 0) { g_create_err = "bg_sim_score_batch: bad arguments"; return BG_E_ARG; }
  if (m == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  BgDev d;
  uint32_t* scratch = nullptr;
  int rc = bg_batch_dev(d, m, &scratch);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(d.err, 0, 4 * sizeof(uint32_t), s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bg_sim_score_batch_kernel, dim3((m + BG_BLOCK - 1) / BG_BLOCK), dim3(BG_BLOCK), 0, s, d, cases_dev, out_dev);
    e = hipGetLastError();
  }
  uint32_t errw = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&errw, d.err, sizeof(errw), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (e != hipSuccess) { g_create_err = std::string("bg_sim_score_batch: ") + hipGetErrorString(e); return BG_E_HIP; }
  if (errw) { g_create_err = "bg_sim_score_batch: a case drew more than two blocks of the global stream"; return BG_E_INTERNAL; }
  return 0;
}

#endif  // BG_ROWS_API_H

// packed records -> the first layer behind BalatroFeaturesExtractor's 447-column input and its weight / bias gradient (bg_extractor.h): entry points of
// their own, so bg_linear_rows keeps refusing the layout.  The header is read here, behind every other kernel of the library, and its kernels are all
// templates: the compiler numbers a function's labels by its place in the module, so kernels added at the end leave the text of the others as it was
// (tools/isa_diff.py).
extern "C++" {
#include "bg_extractor.h"
}
static const BgFirstLayer bg_extractor_layer = {BG_EXT_K, "weight_stride_elems must be in [447, 2**24]", "dweight_stride_elems must be >= 447",
                                                "workspace_dev must be a 16-byte aligned device buffer of bg_extractor_rows_workspace_bytes(m, H) bytes",
                                                bg_extractor_rows_workspace_bytes};

int bg_extractor_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, const void* weight_dev,
                      uint64_t weight_stride_elems, const float* bias_dev, int H, int activation, int out_dtype, void* out_dev, uint64_t out_stride_elems,
                      float* kernel_ms_out, void* stream) {
  const char* bad = bg_first_common_args(rows_dev, row_stride_bytes, store_rows, index_dev, m, H, activation);
  if (!bad) bad = bg_first_forward_args(bg_extractor_layer, rows_dev, index_dev, nullptr, nullptr, weight_dev, weight_stride_elems, bias_dev, H, out_dtype, out_dev, out_stride_elems);
  if (int rc = bg_op_begin("bg_extractor_rows: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const unsigned gx = (unsigned)bg_lin_blocks(m), ys = bg_first_ysplit(gx, H);
  hipStream_t s = (hipStream_t)stream;
  const int relu = activation == BG_LIN_RELU;
  return bg_op_run(kernel_ms_out, s, [&] {
    auto go = [&](auto F32) {
      hipLaunchKernelGGL((bg_extractor_rows_kernel<F32() ? BG_ENC_F32 : BG_ENC_BF16>), dim3(gx, ys), dim3(BG_LIN_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, (const uint16_t*)weight_dev, weight_stride_elems, bias_dev, H, relu, out_dev, out_stride_elems);
    };
    if (out_dtype == BG_ENC_F32) go(std::true_type{}); else go(std::false_type{});
  });
}

uint64_t bg_extractor_rows_workspace_bytes(int64_t m, int H) { return bg_ext_workspace_bytes(m, H); }

int bg_extractor_rows_grad(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows, const int32_t* index_dev, int64_t m, const void* dout_dev,
                           int dout_dtype, uint64_t dout_stride_elems, const void* out_dev, int out_dtype, uint64_t out_stride_elems, int H, int activation,
                           float* dweight_dev, uint64_t dweight_stride_elems, float* dbias_dev, void* workspace_dev, uint64_t workspace_bytes,
                           float* kernel_ms_out, void* stream) {
  const bool relu = activation == BG_LIN_RELU;
  const char* bad = bg_first_common_args(rows_dev, row_stride_bytes, store_rows, index_dev, m, H, activation);
  if (!bad) bad = bg_first_grad_args(bg_extractor_layer, rows_dev, m, dout_dev, dout_dtype, dout_stride_elems, out_dev, out_dtype, out_stride_elems, H, activation, dweight_dev, dweight_stride_elems, dbias_dev, workspace_dev, workspace_bytes);
  if (int rc = bg_op_begin("bg_extractor_rows_grad: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const long long per = bg_ext_blocks_per_group(m, H), groups = bg_ext_groups(m, H);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    const int outk = !relu ? 0 : out_dtype == BG_ENC_F32 ? 1 : 2;
    bg_enc_pick<0, 1, 2>(outk, [&](auto OUTK) {
      auto go = [&](auto DBF16) {
        hipLaunchKernelGGL((bg_extractor_rows_grad_kernel<DBF16(), OUTK()>), dim3((unsigned)groups, (unsigned)bg_lin_spans(H), BG_EXT_KSPANS), dim3(BG_LIN_BLOCK), 0, s, rows_dev, row_stride_bytes, index_dev, (long long)store_rows, (long long)m, dout_dev, dout_stride_elems, out_dev, out_stride_elems, H, per, (float*)workspace_dev);
      };
      if (dout_dtype == BG_ENC_BF16) go(std::true_type{}); else go(std::false_type{});
    });
    const long long items = (long long)BG_EXT_PART_ROWS * H;
    hipLaunchKernelGGL((bg_extractor_reduce_kernel<BG_EXT_K>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const float*)workspace_dev, groups, H, dweight_dev, dweight_stride_elems, dbias_dev);
  });
}

// the last hidden activation -> the policy's last layer fused with the masked head and with PPO's loss (bg_actor.h).  Read here for the reason given
// above bg_extractor.h: kernels added behind every other leave the text of the others as it was.
extern "C++" {
#include "bg_actor.h"
}
// what the three calls check of (h, Hin, weight, bias, logits_out), behind their own shape checks
static const char* bg_actor_layer_args(const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems,
                                       const float* bias_dev, const float* logits_out_dev, uint64_t logits_out_stride_elems) {
  if (!bg_act_hin_ok(Hin)) return "Hin must be a multiple of 32 in [32, 1024]";
  if (bg_head_bad_h(h_dev)) return "h_dev must be a 16-byte aligned device pointer";
  if (bg_head_bad_h_stride(h_stride_elems, (uint64_t)Hin)) return "h_stride_elems must be a multiple of 8, >= Hin";
  if (weight_dtype != BG_ENC_F32 && weight_dtype != BG_ENC_BF16) return "weight_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  if (!weight_dev || ((uintptr_t)weight_dev & (weight_dtype == BG_ENC_F32 ? 3 : 1))) return "weight_dev must be a device pointer aligned to its element type";
  if (weight_stride_elems < (uint64_t)Hin || weight_stride_elems > 0xffffffffull) return "weight_stride_elems must be >= Hin";
  if ((uintptr_t)bias_dev & 3) return "bias_dev must be 4-byte aligned";
  return bg_head_logits_out_args(logits_out_dev, logits_out_stride_elems);
}
static BgActorArgs bg_actor_args(const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems,
                                 const float* bias_dev, float* logits_out_dev, uint64_t logits_out_stride_elems) {
  BgActorArgs G;
  G.h = (const uint16_t*)h_dev; G.hstride = h_stride_elems; G.weight = weight_dev; G.wstride = weight_stride_elems; G.w_bf16 = weight_dtype == BG_ENC_BF16 ? 1 : 0;
  G.bias = bias_dev; G.Hin = Hin; G.logits_out = logits_out_dev; G.lostride = logits_out_stride_elems;
  G.lost = bg_head_logits_out_path(logits_out_dev, logits_out_stride_elems);
  return G;
}

static int bg_actor_head_call(const char* who, int mode, const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype,
                              uint64_t weight_stride_elems, const float* bias_dev, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m, uint64_t seed,
                              uint64_t index0, uint64_t t, const int32_t* actions_in, int32_t* actions_out, float* log_prob_dev, float* entropy_dev,
                              float* logits_out_dev, uint64_t logits_out_stride_elems, float* kernel_ms_out, void* stream) {
  const void* const act = mode == BG_HEAD_EVALUATE ? (const void*)actions_in : (const void*)actions_out;
  const void* const ins[] = {h_dev, weight_dev, bias_dev, mask_dev, mode == BG_HEAD_EVALUATE ? act : nullptr};
  const void* const outs[] = {mode == BG_HEAD_EVALUATE ? nullptr : act, log_prob_dev, entropy_dev, logits_out_dev};
  const char* bad = bg_head_shape_args(BG_HEAD_F32, m);
  if (bad) {}
  else if (const char* r = bg_actor_layer_args(h_dev, h_stride_elems, Hin, weight_dev, weight_dtype, weight_stride_elems, bias_dev, logits_out_dev, logits_out_stride_elems)) bad = r;
  else if (const char* r = bg_head_mask_args(mask_dev, mask_stride_bytes)) bad = r;
  else if (const char* r = bg_head_out_args(act, log_prob_dev, entropy_dev)) bad = r;
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin(who, bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const BgActorArgs G = bg_actor_args(h_dev, h_stride_elems, Hin, weight_dev, weight_dtype, weight_stride_elems, bias_dev, logits_out_dev, logits_out_stride_elems);
  const int mld = bg_head_mask_path(mask_dev, mask_stride_bytes, true);
  const unsigned grid = (unsigned)bg_act_blocks(m);
  const uint64_t wes = weight_dtype == BG_ENC_BF16 ? 2u : 4u;
  const int wvec = ((uintptr_t)weight_dev & 15) == 0 && (weight_stride_elems * wes) % 16 == 0 ? BG_ACT_W_VEC : 0;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_enc_pick<BG_HEAD_SAMPLE, BG_HEAD_ARGMAX, BG_HEAD_EVALUATE>(mode, [&](auto M) {
      hipLaunchKernelGGL((bg_actor_head_kernel<M()>), dim3(grid), dim3(BG_HEAD_BLOCK), 0, s, G, wvec, mask_dev, mld, mask_stride_bytes, (long long)m, seed, index0, t, actions_in, actions_out, log_prob_dev, entropy_dev);
    });
  });
}

int bg_actor_sample(const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems,
                    const float* bias_dev, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m, uint32_t flags, uint64_t seed, uint64_t index0,
                    uint64_t t, int32_t* actions_dev, float* log_prob_dev, float* entropy_dev, float* logits_out_dev, uint64_t logits_out_stride_elems,
                    float* kernel_ms_out, void* stream) {
  if (flags & ~BG_HEAD_DETERMINISTIC) { g_create_err = "bg_actor_sample: flags must be 0 or BG_HEAD_DETERMINISTIC"; return BG_E_ARG; }
  return bg_actor_head_call("bg_actor_sample: ", bg_head_mode(flags), h_dev, h_stride_elems, Hin, weight_dev, weight_dtype,
                            weight_stride_elems, bias_dev, mask_dev, mask_stride_bytes, m, seed, index0, t, nullptr, actions_dev, log_prob_dev, entropy_dev,
                            logits_out_dev, logits_out_stride_elems, kernel_ms_out, stream);
}
int bg_actor_evaluate(const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems,
                      const float* bias_dev, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m, const int32_t* actions_dev, float* log_prob_dev,
                      float* entropy_dev, float* logits_out_dev, uint64_t logits_out_stride_elems, float* kernel_ms_out, void* stream) {
  return bg_actor_head_call("bg_actor_evaluate: ", BG_HEAD_EVALUATE, h_dev, h_stride_elems, Hin, weight_dev, weight_dtype, weight_stride_elems, bias_dev, mask_dev,
                            mask_stride_bytes, m, 0, 0, 0, actions_dev, nullptr, log_prob_dev, entropy_dev, logits_out_dev, logits_out_stride_elems, kernel_ms_out, stream);
}

uint64_t bg_actor_ppo_loss_workspace_bytes(int64_t m, int Hin) { return bg_act_workspace_bytes(m, Hin); }
// the rows one group accumulates in float32 before the float64 sum over the groups (what bounds dweight's and dbias' rounding); 0 for a refused shape
int64_t bg_actor_ppo_loss_rows_per_group(int64_t m, int Hin) { return m > 0 && bg_act_hin_ok(Hin) ? bg_act_blocks_per_group(m, Hin) * BG_ACT_ROWS : 0; }

int bg_actor_ppo_loss(const void* h_dev, uint64_t h_stride_elems, int Hin, const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems,
                      const float* bias_dev, const int8_t* mask_dev, uint64_t mask_stride_bytes, const int32_t* actions_dev, const float* old_log_prob_dev,
                      const float* advantages_dev, const float* values_dev, const float* returns_dev, const int32_t* index_dev, int64_t store_rows, int64_t m,
                      float clip_range, float ent_coef, float vf_coef, uint32_t flags, void* dh_dev, int dh_dtype, uint64_t dh_stride_elems, float* dweight_dev,
                      float* dbias_dev, float* dvalues_dev, float* log_prob_dev, float* entropy_dev, float* stats_dev, float* logits_out_dev,
                      uint64_t logits_out_stride_elems, float* dlogits_out_dev, uint64_t dlogits_out_stride_elems, void* workspace_dev, uint64_t workspace_bytes,
                      float* kernel_ms_out, void* stream) {
  const void* const ins[] = {h_dev, weight_dev, bias_dev, mask_dev, actions_dev, old_log_prob_dev, advantages_dev, values_dev, returns_dev, index_dev};
  const void* const outs[] = {dh_dev, dweight_dev, dbias_dev, dvalues_dev, log_prob_dev, entropy_dev, stats_dev, logits_out_dev, dlogits_out_dev, workspace_dev};
  const BgPpoStored S = {mask_dev, mask_stride_bytes, actions_dev, old_log_prob_dev, advantages_dev, values_dev, returns_dev, index_dev, store_rows,
                         dvalues_dev, log_prob_dev, entropy_dev, stats_dev};
  const uint64_t ds = dh_dtype == BG_ENC_F32 ? 4u : 2u;
  const char* bad = bg_head_shape_args(BG_HEAD_F32, m);
  if (bad) {}
  else if (const char* r = bg_ppo_coef_args(flags, clip_range, ent_coef, vf_coef)) bad = r;
  else if (const char* r = bg_actor_layer_args(h_dev, h_stride_elems, Hin, weight_dev, weight_dtype, weight_stride_elems, bias_dev, logits_out_dev, logits_out_stride_elems)) bad = r;
  else if (dh_dtype != BG_ENC_F32 && dh_dtype != BG_ENC_BF16) bad = "dh_dtype must be BG_ENC_F32 or BG_ENC_BF16";
  else if (!dh_dev || ((uintptr_t)dh_dev & (ds - 1))) bad = "dh_dev must be a device pointer aligned to its element type";
  else if (dh_stride_elems < (uint64_t)Hin || dh_stride_elems > 0xffffffffull) bad = "dh_stride_elems must be >= Hin";
  else if (!dweight_dev || !dbias_dev || (((uintptr_t)dweight_dev | (uintptr_t)dbias_dev) & 3)) bad = "dweight_dev and dbias_dev must be 4-byte aligned device pointers";
  else if ((uintptr_t)dlogits_out_dev & 3) bad = "dlogits_out_dev must be 4-byte aligned";
  else if (dlogits_out_dev && (dlogits_out_stride_elems < BG_HEAD_ACTIONS || dlogits_out_stride_elems > 0xffffffffull)) bad = "dlogits_out_stride_elems must be >= 60";
  else if (const char* r = bg_ppo_stored_args(S)) bad = r;
  else if (bg_loss_bad_workspace(m, workspace_dev, workspace_bytes, bg_act_workspace_bytes(m, Hin))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_actor_ppo_loss_workspace_bytes(m, Hin) bytes";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_actor_ppo_loss: ", bad, kernel_ms_out)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) {
    BG_HIP0(hipMemsetAsync(dweight_dev, 0, (size_t)BG_HEAD_ACTIONS * Hin * sizeof(float), s));
    BG_HIP0(hipMemsetAsync(dbias_dev, 0, BG_HEAD_ACTIONS * sizeof(float), s));
    return bg_loss_empty(stats_dev, BG_PPO_STATS, s);
  }
  const BgActorArgs G = bg_actor_args(h_dev, h_stride_elems, Hin, weight_dev, weight_dtype, weight_stride_elems, bias_dev, logits_out_dev, logits_out_stride_elems);
  BgPpoArgs A = bg_ppo_args(S, m, clip_range, ent_coef, vf_coef, flags, workspace_dev);
  A.logits = nullptr; A.lstride = 0; A.lld = BG_HEAD_LD_WORD;
  A.dlogits = dlogits_out_dev; A.dstride = dlogits_out_stride_elems; A.dst = dlogits_out_dev ? bg_head_ld_path(dlogits_out_dev, dlogits_out_stride_elems, false) : BG_HEAD_LD_WORD;
  BgActorGrad R;
  R.dh = dh_dev; R.dhstride = dh_stride_elems; R.dh_bf16 = dh_dtype == BG_ENC_BF16 ? 1 : 0;
  R.part = (float*)((uint8_t*)workspace_dev + bg_act_ppo_ws_bytes(m)); R.per = bg_act_blocks_per_group(m, Hin);
  const long long groups = bg_act_groups(m, Hin);
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_ppo_launch_adv(A, s);
    hipLaunchKernelGGL((bg_actor_ppo_kernel<BG_PPO_SUMS>), dim3((unsigned)groups, (unsigned)bg_act_spans(Hin)), dim3(BG_ACT_BLOCK), 0, s, A, G, R);
    bg_ppo_launch_finish(A, stats_dev, s);
    const long long items = (long long)BG_HEAD_ACTIONS * Hin + BG_HEAD_ACTIONS;
    hipLaunchKernelGGL((bg_actor_reduce_kernel<BG_HEAD_ACTIONS>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const float*)R.part, groups, Hin, dweight_dev, dbias_dev);
  });
}

// every parameter tensor's gradient -> the clipped Adam / RMSpropTFLike step, the bfloat16 shadows, DQN's target update and the zeroing (bg_optim.h).
// Read here, behind every other header, for the reason given above bg_extractor.h.
extern "C++" {
#include "bg_optim.h"
}
uint64_t bg_optim_workspace_size(int64_t chunks) { return bg_optim_ws_bytes((long long)chunks); }

int bg_optim_step(const void* table_dev, int ntensors, int64_t chunks, int algo, double lr, double beta1, double beta2, double eps, double weight_decay,
                  double max_norm, double tau, uint32_t flags, void* carry_dev, void* workspace_dev, void* stats_dev, float* kernel_ms_out, void* stream) {
  const bool shadow_only = (flags & BG_OPTIM_SHADOW_ONLY) != 0u;
  const char* bad = nullptr;
  if (ntensors < 0 || ntensors > BG_OPTIM_MAX_TENSORS) bad = "ntensors must be in [0, 1024]";
  else if (chunks < 0 || chunks > 0x7fffffffll || (ntensors == 0) != (chunks == 0) || chunks < ntensors) bad = "chunks must be the table's chunk count: in [ntensors, 2**31), 0 for an empty table";
  else if (algo != BG_OPTIM_ADAM && algo != BG_OPTIM_RMSPROP_TF) bad = "algo must be BG_OPTIM_ADAM or BG_OPTIM_RMSPROP_TF";
  else if (flags & ~(BG_OPTIM_ZERO_GRAD | BG_OPTIM_SHADOW_ONLY)) bad = "flags must be a combination of BG_OPTIM_ZERO_GRAD and BG_OPTIM_SHADOW_ONLY";
  else if (!(lr >= 0.0 && lr < 1e30)) bad = "lr must be finite and >= 0";
  else if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) bad = "beta1 (alpha) and beta2 must be in [0, 1)";
  else if (!(eps >= 0.0 && eps < 1e30) || !(weight_decay >= 0.0 && weight_decay < 1e30)) bad = "eps and weight_decay must be finite and >= 0";
  else if (!(max_norm < 1e30)) bad = "max_norm must be a number below 1e30 (<= 0: no clipping)";
  else if (!(tau >= 0.0 && tau <= 1.0)) bad = "tau must be in [0, 1]";
  else if (ntensors && (!table_dev || ((uintptr_t)table_dev & 15))) bad = "table_dev must be a 16-byte aligned device pointer";
  else if (ntensors && !shadow_only && (!carry_dev || ((uintptr_t)carry_dev & 7))) bad = "carry_dev must be an 8-byte aligned device pointer to 32 bytes";
  else if (ntensors && !shadow_only && (!workspace_dev || ((uintptr_t)workspace_dev & 15))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_optim_workspace_size(chunks) bytes";
  else if (ntensors && !shadow_only && (!stats_dev || ((uintptr_t)stats_dev & 7))) bad = "stats_dev must be an 8-byte aligned device pointer to BG_OPTIM_STATS_BYTES bytes";
  else if (ntensors && !shadow_only && (carry_dev == stats_dev || carry_dev == workspace_dev || stats_dev == workspace_dev || table_dev == carry_dev || table_dev == workspace_dev || table_dev == stats_dev)) bad = "table, carry, workspace and stats must be four different buffers";
  if (int rc = bg_op_begin("bg_optim_step: ", bad, kernel_ms_out)) return rc;
  if (ntensors == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const BgOptHyper h = bg_optim_hyper(algo, lr, beta1, beta2, eps, weight_decay, max_norm, tau, flags);
  const BgOptTensor* const table = (const BgOptTensor*)table_dev;
  BgOptHead* const head = (BgOptHead*)workspace_dev;
  BgOptPart* const part = (BgOptPart*)((uint8_t*)workspace_dev + BG_OPT_WS_HEAD);
  const dim3 grid((unsigned)chunks), block(BG_OPT_LANES);
  return bg_op_run(kernel_ms_out, s, [&] {
    if (shadow_only) {
      hipLaunchKernelGGL((bg_optim_update<BG_OPTIM_ADAM, true>), grid, block, 0, s, table, ntensors, h, (const BgOptHead*)nullptr);
      return;
    }
    hipLaunchKernelGGL((bg_optim_norm_partials<BG_OPT_LANES>), grid, block, 0, s, table, ntensors, part);
    hipLaunchKernelGGL((bg_optim_combine<BG_OPT_LANES>), dim3(1), block, 0, s, (const BgOptPart*)part, (long long)chunks, h, (BgOptCarry*)carry_dev, head, (BgOptStats*)stats_dev);
    if (algo == BG_OPTIM_ADAM) hipLaunchKernelGGL((bg_optim_update<BG_OPTIM_ADAM, false>), grid, block, 0, s, table, ntensors, h, (const BgOptHead*)head);
    else hipLaunchKernelGGL((bg_optim_update<BG_OPTIM_RMSPROP_TF, false>), grid, block, 0, s, table, ntensors, h, (const BgOptHead*)head);
  });
}

// a finished [K + 1, N] store + a weight per candidate row -> the kept demonstration steps compacted into a device ring, and uniform draws over its
// filled slots (bg_demo.h).  Read here, behind every other header, for the reason given above bg_extractor.h.  Workspace: BG_DEMO_WS_HEAD bytes
// (T0 mod capacity, the drop threshold), one uint32 per chunk of 1 024 candidate rows.
extern "C++" {
#include "bg_demo.h"
}
uint64_t bg_demo_workspace_bytes(int64_t store_rows) { return bg_demo_ws_bytes(store_rows); }

// [a, a + an) and [b, b + bn) share a byte
static bool bg_demo_overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
  return (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}

int bg_demo_append_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, const float* weights_dev, const double* returns_dev,
                        uint8_t* demo_dev, uint64_t demo_stride_bytes, int64_t capacity, float* demo_weight_dev, int32_t* demo_source_dev,
                        int64_t* cursor_dev, void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream) {
  const void* const ins[] = {rows_dev, weights_dev, returns_dev};
  const void* const outs[] = {demo_dev, demo_weight_dev, demo_source_dev, cursor_dev, workspace_dev};
  const bool range = N >= 0 && K >= 0 && (N == 0 || (K >= 1 && (uint64_t)K * (uint64_t)N < 0x80000000ull));
  const int64_t M = range ? (int64_t)K * N : 0;
  const char* bad = nullptr;
  if (!range) bad = "K must be >= 1 (with N > 0), N >= 0 and K * N < 2**31";
  else if (capacity < 1 || capacity >= 0x80000000ll) bad = "capacity must be in [1, 2**31)";
  else if (const char* r = bg_rows_args(rows_dev, row_stride_bytes)) bad = r;
  else if (!demo_dev || demo_stride_bytes < BG_ROW_BYTES || (demo_stride_bytes & 15) || ((uintptr_t)demo_dev & 15) || demo_stride_bytes > 0xffffffffull) bad = "demo_dev must be 16-byte aligned and demo_stride_bytes a multiple of 16, >= BG_ROW_BYTES";
  else if (!weights_dev || !demo_weight_dev || !cursor_dev) bad = "weights_dev, demo_weight_dev and cursor_dev must be device pointers";
  else if (((uintptr_t)weights_dev | (uintptr_t)demo_weight_dev | (uintptr_t)demo_source_dev) & 3) bad = "weights_dev, demo_weight_dev and demo_source_dev must be 4-byte aligned";
  else if (((uintptr_t)returns_dev | (uintptr_t)cursor_dev) & 7) bad = "returns_dev and cursor_dev must be 8-byte aligned";
  else if (bg_demo_overlap(rows_dev, ((uint64_t)M + (uint64_t)N) * row_stride_bytes, demo_dev, (uint64_t)capacity * demo_stride_bytes)) bad = "the ring must not overlap the store";
  else if (M > 0 && (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < bg_demo_ws_bytes(M))) bad = "workspace_dev must be a 16-byte aligned device buffer of bg_demo_workspace_bytes(K * N) bytes";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_demo_append_rows: ", bad, kernel_ms_out)) return rc;
  if (M == 0) return 0;
  const int64_t chunks = (int64_t)bg_demo_chunks_of(M);
  int64_t* const head = (int64_t*)workspace_dev;
  uint32_t* const offs = (uint32_t*)((uint8_t*)workspace_dev + BG_DEMO_WS_HEAD);
  BgDemoArgs A;
  A.rows = rows_dev; A.stride = row_stride_bytes; A.N = N; A.M = M;
  A.wbits = (const uint32_t*)weights_dev; A.vec = ((uintptr_t)weights_dev & 15) == 0 ? 1 : 0;
  A.ret_bits = (const uint64_t*)returns_dev;
  A.demo = demo_dev; A.dstride = demo_stride_bytes; A.capacity = capacity;
  A.demo_weight = (uint32_t*)demo_weight_dev; A.demo_source = demo_source_dev;
  A.head = head; A.offs = offs;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    hipLaunchKernelGGL((bg_demo_count_kernel<BG_DEMO_LANES>), dim3((unsigned)chunks), dim3(BG_DEMO_LANES), 0, s, A.wbits, M, A.vec, offs);
    hipLaunchKernelGGL((bg_demo_scan_kernel<BG_DEMO_LANES>), dim3(1), dim3(BG_DEMO_LANES), 0, s, offs, chunks, capacity, cursor_dev, head);
    bg_bool_dispatch(returns_dev != nullptr, false, [&](auto R, auto) {
      hipLaunchKernelGGL((bg_demo_scatter_kernel<R(), BG_DEMO_NT != 0>), dim3((unsigned)chunks), dim3(BG_DEMO_LANES), 0, s, A);
    });
  });
}

int bg_demo_sample(const int64_t* cursor_dev, int64_t capacity, uint64_t seed, uint64_t index0, uint64_t t, int32_t* index_dev, int64_t m,
                   float* kernel_ms_out, void* stream) {
  const char* bad = nullptr;
  if (m < 0 || m > (int64_t)BG_DEMO_LANES * 0x7fffffffll) bad = "m out of range";
  else if (capacity < 1 || capacity >= 0x80000000ll) bad = "capacity must be in [1, 2**31)";
  else if (!cursor_dev || ((uintptr_t)cursor_dev & 7)) bad = "cursor_dev must be an 8-byte aligned device pointer to int64[2]";
  else if (!index_dev || ((uintptr_t)index_dev & 3)) bad = "index_dev must be a 4-byte aligned device pointer";
  else if ((const void*)cursor_dev == (const void*)index_dev) bad = "index_dev must not be the same pointer as cursor_dev";
  if (int rc = bg_op_begin("bg_demo_sample: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    hipLaunchKernelGGL((bg_demo_sample_kernel<BG_DEMO_LANES>), dim3((unsigned)((m + BG_DEMO_LANES - 1) / BG_DEMO_LANES)), dim3(BG_DEMO_LANES), 0, s, cursor_dev, capacity, seed, index0, t, index_dev, m);
  });
}

// packed records -> the scripted expert's action per record (bg_expert.h): stateless, one launch, one store per output per record.  Read here, behind
// every other header, for the reason given above bg_extractor.h.  lanes_per_record: the lane group that shares a record's subsets
// (bg_expert_kernel<G>); 0 = bg_expert_lanes(m), the measured choice.
extern "C++" {
#include "bg_expert.h"
}
int bg_expert_actions_ex(const void* rows_dev, int64_t row_stride_bytes, int64_t m, const int32_t* index_dev, int64_t store_rows, int32_t* actions_dev,
                         int32_t* detail_dev, int lanes_per_record, float* kernel_ms_out, void* stream) {
  const void* const ins[] = {rows_dev, index_dev};
  const void* const outs[] = {actions_dev, detail_dev};
  const uint64_t span = store_rows > 0 && row_stride_bytes > 0 ? (uint64_t)store_rows * (uint64_t)row_stride_bytes : 0;
  const char* bad = nullptr;
  if (m < 0 || m >= 0x80000000ll) bad = "m must be in [0, 2**31)";
  else if (store_rows < 0 || store_rows > 0x7fffffffffffll) bad = "store_rows must be in [0, 2**47)";
  else if (index_dev && store_rows > 0x7fffffffll) bad = "store_rows must be in [0, 2**31) when index_dev is given";
  else if (!index_dev && m > store_rows) bad = "m must be <= store_rows when index_dev is NULL";
  else if (row_stride_bytes < 0) bad = "rows_dev must be 16-byte aligned and row_stride_bytes a multiple of 16, >= BG_ROW_BYTES";
  else if (const char* r = bg_rows_args(rows_dev, (uint64_t)row_stride_bytes)) bad = r;
  else if ((uintptr_t)index_dev & 3) bad = "index_dev must be 4-byte aligned";
  else if (!actions_dev || (((uintptr_t)actions_dev | (uintptr_t)detail_dev) & 3)) bad = "actions_dev must be a 4-byte aligned device pointer (detail_dev 4-byte aligned)";
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as each other";
  else if (bg_demo_overlap(rows_dev, span, actions_dev, (uint64_t)m * 4u) || (detail_dev && bg_demo_overlap(rows_dev, span, detail_dev, (uint64_t)m * 4u))) bad = "outputs must not overlap the records";
  else if (lanes_per_record != 0 && lanes_per_record != 1 && lanes_per_record != 8 && lanes_per_record != 64) bad = "lanes_per_record must be 0, 1, 8 or 64";
  if (int rc = bg_op_begin("bg_expert_actions: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  const int G = lanes_per_record ? lanes_per_record : bg_expert_lanes(m);
  const unsigned grid = (unsigned)(((uint64_t)m * (uint64_t)G + BG_EXPERT_BLOCK - 1) / BG_EXPERT_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_enc_pick<1, 8, 64>(G, [&](auto LG) {
      bg_bool_dispatch(detail_dev != nullptr, false, [&](auto D, auto) {
        hipLaunchKernelGGL((bg_expert_kernel<LG(), D()>), dim3(grid), dim3(BG_EXPERT_BLOCK), 0, s, (const uint8_t*)rows_dev, (uint64_t)row_stride_bytes, (long long)m, index_dev, (long long)store_rows, actions_dev, detail_dev);
      });
    });
  });
}
int bg_expert_actions(const void* rows_dev, int64_t row_stride_bytes, int64_t m, const int32_t* index_dev, int64_t store_rows, int32_t* actions_dev,
                      int32_t* detail_dev, void* stream) {
  return bg_expert_actions_ex(rows_dev, row_stride_bytes, m, index_dev, store_rows, actions_dev, detail_dev, 0, nullptr, stream);
}

// the first layer's output -> every hidden layer, action_net, the masked head and value_net in one launch (bg_policy.h).  Read here, behind every other
// header, for the reason given above bg_extractor.h.  The net is a HOST table: checked on every call, carried to the kernel as a launch argument.
extern "C++" {
#include "bg_policy.h"
}
static_assert(sizeof(BgPolicyLayer) == sizeof(BgPolLayer) && sizeof(BgPolicyNet) == sizeof(BgPolNet) && offsetof(BgPolicyNet, layer) == offsetof(BgPolNet, layer) &&
              offsetof(BgPolicyLayer, weight_stride_elems) == offsetof(BgPolLayer, wpitch) && offsetof(BgPolicyLayer, out_features) == offsetof(BgPolLayer, out) &&
              offsetof(BgPolicyLayer, activation) == offsetof(BgPolLayer, act), "bg_policy.h reads the header's table");
static_assert(BG_POLICY_ACT_NONE == BG_POL_NONE && BG_POLICY_ACT_RELU == BG_POL_RELU && BG_POLICY_ACT_TANH == BG_POL_TANH && BG_POLICY_MAX_LAYERS == BG_POL_LAYERS_MAX &&
              BG_POLICY_MAX_SECTION == BG_POL_SECTION_MAX && BG_POLICY_MAX_WIDTH == BG_POL_WMAX, "the header's constants");

int bg_policy_check(const BgPolicyNet* net) {
  if (const char* r = bg_pol_check((const BgPolNet*)net)) { g_create_err = std::string("bg_policy_check: ") + r; return BG_E_ARG; }
  return 0;
}
int bg_policy_tap_cols(const BgPolicyNet* net) {
  if (bg_policy_check(net)) return BG_E_ARG;
  return bg_pol_tap_cols(*(const BgPolNet*)net);
}

int bg_policy_forward(const BgPolicyNet* net, const void* h_dev, uint64_t h_stride_elems, const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m,
                      uint32_t flags, uint64_t seed, uint64_t index0, uint64_t t, int32_t* actions_dev, float* log_prob_dev, float* entropy_dev, float* values_dev,
                      void* taps_dev, uint64_t taps_stride_elems, float* logits_out_dev, uint64_t logits_out_stride_elems, float* kernel_ms_out, void* stream) {
  const BgPolNet* const N = (const BgPolNet*)net;
  const bool evaluate = (flags & BG_POLICY_EVALUATE) != 0u;
  const void* const ins[] = {h_dev, mask_dev, evaluate ? (const void*)actions_dev : nullptr};
  const void* const outs[] = {evaluate ? nullptr : (const void*)actions_dev, log_prob_dev, entropy_dev, values_dev, taps_dev, logits_out_dev};
  const char* bad = bg_pol_check(N);
  if (bad) {}
  else if ((flags & ~(BG_HEAD_DETERMINISTIC | BG_POLICY_EVALUATE)) || flags == (BG_HEAD_DETERMINISTIC | BG_POLICY_EVALUATE)) bad = "flags must be 0, BG_HEAD_DETERMINISTIC or BG_POLICY_EVALUATE";
  else if (m < 0 || m > (int64_t)BG_POL_ROWS * 0x7fffffffll) bad = "m out of range";
  else if (bg_head_bad_h(h_dev)) bad = "h_dev must be a 16-byte aligned device pointer";
  else if (bg_head_bad_h_stride(h_stride_elems, N->in0)) bad = "h_stride_elems must be a multiple of 8, >= in0";
  else if (const char* r = bg_head_mask_args(mask_dev, mask_stride_bytes)) bad = r;
  else if (const char* r = bg_head_out_args(actions_dev, nullptr, nullptr)) bad = r;   // (log_prob / entropy: with values_dev, below)
  else if (((uintptr_t)log_prob_dev | (uintptr_t)entropy_dev | (uintptr_t)values_dev) & 3) bad = "log_prob_dev / entropy_dev / values_dev must be 4-byte aligned";
  else if (values_dev && !N->has_value) bad = "values_dev needs the value layer (has_value)";
  else if ((uintptr_t)taps_dev & 1) bad = "taps_dev must be 2-byte aligned";
  else if (taps_dev && (taps_stride_elems < (uint64_t)bg_pol_tap_cols(*N) || taps_stride_elems > 0xffffffffull)) bad = "taps_stride_elems must be >= bg_policy_tap_cols(net)";
  else if (const char* r = bg_head_logits_out_args(logits_out_dev, logits_out_stride_elems)) bad = r;
  else if (bg_alias(ins, outs)) bad = "outputs must not be the same pointer as an input or as another output";
  if (int rc = bg_op_begin("bg_policy_forward: ", bad, kernel_ms_out)) return rc;
  if (m == 0) return 0;
  BgPolIo O;
  O.h = (const uint16_t*)h_dev; O.hstride = h_stride_elems;
  O.mask = mask_dev; O.mstride = mask_stride_bytes; O.mld = bg_head_mask_path(mask_dev, mask_stride_bytes, true);
  O.m = (long long)m; O.seed = seed; O.index0 = index0; O.t = t;
  O.actions_in = evaluate ? actions_dev : nullptr; O.actions_out = evaluate ? nullptr : actions_dev;
  O.log_prob = log_prob_dev; O.entropy = entropy_dev; O.values = values_dev;
  O.taps = (uint16_t*)taps_dev; O.tstride = taps_stride_elems;
  O.logits_out = logits_out_dev; O.lostride = logits_out_stride_elems;
  O.lost = bg_head_logits_out_path(logits_out_dev, logits_out_stride_elems);
  const int mode = bg_head_mode(flags, evaluate);
  const unsigned grid = (unsigned)((m + BG_POL_ROWS - 1) / BG_POL_ROWS);
  const BgPolNet net_arg = *N;
  hipStream_t s = (hipStream_t)stream;
  return bg_op_run(kernel_ms_out, s, [&] {
    bg_enc_pick<BG_HEAD_SAMPLE, BG_HEAD_ARGMAX, BG_HEAD_EVALUATE>(mode, [&](auto M) {
      hipLaunchKernelGGL((bg_policy_kernel<M()>), dim3(grid), dim3(BG_POL_BLOCK), 0, s, net_arg, O);
    });
  });
}
