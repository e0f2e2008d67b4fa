/*
 * sel.h — C ABI of libsel.so, the MI355X (gfx950) kernels behind the
 * denoise-training hot path of s194584/dl-speech-enhancement.
 *
 * Conventions (all entry points):
 *   - every pointer is caller-owned DEVICE memory, contiguous, fp32 unless the
 *     name says otherwise; the library never allocates device memory — scratch
 *     comes in through (ws, ws_bytes) sized by the matching *_workspace() call;
 *   - work is only enqueued on `stream` (no host sync); functions are stateless
 *     and reentrant after sel_init();
 *   - return 0 on success or a negative SEL_ERR_* code; sel_last_error() gives
 *     a thread-local message.  Nothing throws across the ABI.
 *
 * The reference has no native API (it is pure PyTorch); each entry point names
 * the reference function it replaces (file:line under the reference root).
 */
#ifndef SEL_H_
#define SEL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* sel_stream_t; /* == hipStream_t */

enum {
  SEL_OK = 0,
  SEL_ERR_ARG = -1,         /* bad shape / size / pointer */
  SEL_ERR_HIP = -2,         /* HIP runtime error */
  SEL_ERR_UNSUPPORTED = -3, /* legal for the reference but not implemented */
  SEL_ERR_WORKSPACE = -4,   /* workspace too small */
  SEL_ERR_STATE = -5        /* sel_init() not called / failed */
};

enum { SEL_LOG_E = 0, SEL_LOG_2 = 1, SEL_LOG_10 = 2 };

/* ---- library ---------------------------------------------------------- */
int sel_init(void);                 /* uploads FFT twiddle tables; idempotent */
const char* sel_last_error(void);   /* thread-local, never NULL */
int sel_version(void);
/* tuning knobs for A/B runs inside one process (keys 0..127; key 0: conv fwd
 * kernel variant, 0 = built-in heuristic); returns the previous value, -1 for a
 * key out of range (the call then changes nothing). */
int sel_tune(int key, int value);
/* current value of a tuning knob, read-only (-1 for a key out of range). */
int sel_tune_get(int key);
/* diagnostics: out[2i], out[2i+1] = raw_buffer_load_b64 of x at byte offset 4i
 * (i < n-1) through the STFT kernels' buffer resource (spectral.hip fetch_frame);
 * mode 0: elements taken as scalars, mode 1: __builtin_bit_cast of the vector
 * elements (miscompiled by ROCm 7.2 clang: element 0 twice) */
int sel_probe_buffer_b64(const float* x, int n, int mode, float* out, sel_stream_t stream);
/* measurement: copy n16 16-byte elements (float4) src -> dst with `blocks`
 * workgroups striding over the buffer (the HBM copy-rate denominator of the
 * STFT roofline in bench.py) */
int sel_probe_copy_f4(const void* src, void* dst, int64_t n16, int blocks, sel_stream_t stream);

/* ---- STFT magnitude: losses/stft_loss.py:19-35 (stft) ------------------
 * x (B,T) -> mag (B, F, K), F = 1 + T/hop, K = n_fft/2 + 1.
 * torch.stft semantics: center=True, reflect pad n_fft/2, periodic window of
 * win_length zero-padded centred to n_fft, onesided, unnormalised;
 * mag = sqrt(max(re^2 + im^2, pow_floor)).  n_fft in {256..4096}, power of 2. */
int sel_stft_mag_fwd(const float* x, int64_t B, int64_t T, int n_fft, int hop,
                     int win_length, const float* window, float pow_floor,
                     float* mag, sel_stream_t stream);
/* grad: g_x (B,T) from g_mag (B,F,K).  Overwrites g_x. */
size_t sel_stft_bwd_workspace(int64_t B, int64_t T, int n_fft, int hop, int win_length);
int sel_stft_mag_bwd(const float* x, int64_t B, int64_t T, int n_fft, int hop,
                     int win_length, const float* window, float pow_floor,
                     const float* g_mag, float* g_x, void* ws, size_t ws_bytes,
                     sel_stream_t stream);

/* ---- SC + log-magnitude reductions on magnitudes -----------------------
 * losses/stft_loss.py:45-56 (SpectralConvergenceLoss), :66-77 (LogSTFTMagnitudeLoss).
 * sums (3 doubles, device) = { sum (y-x)^2, sum y^2, sum |ln y - ln x| } over n. */
size_t sel_mag_pair_workspace(int64_t n);
int sel_mag_pair_sums(const float* x_mag, const float* y_mag, int64_t n,
                      double* sums, void* ws, size_t ws_bytes, sel_stream_t stream);
/* coef (device, 4 floats) = {a, b, c, d}:
 *   g_x = a*(x - y) + b*sign(ln x - ln y)/x
 *   g_y = c*(y - x) + d*y + b*sign(ln y - ln x)/y      (g_y may be NULL)  */
int sel_mag_pair_bwd(const float* x_mag, const float* y_mag, int64_t n, const float* coef,
                     float* g_x, float* g_y, sel_stream_t stream);

/* ---- fused STFT loss for one resolution: losses/stft_loss.py:100-117 ---
 * Computes both STFTs per frame in LDS, never writes magnitudes.
 * sums (3 doubles) as sel_mag_pair_sums.  bwd: coef (device, 2 floats) = {a, b},
 * g_x = dL/dx through g_xmag = a*(xm - ym) + b*sign(ln xm - ln ym)/xm. */
size_t sel_stft_loss_workspace(int64_t B, int64_t T, int n_fft, int hop, int win_length);
int sel_stft_loss_fwd(const float* x, const float* y, int64_t B, int64_t T, int n_fft,
                      int hop, int win_length, const float* window, double* sums,
                      void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_stft_loss_bwd(const float* x, const float* y, int64_t B, int64_t T, int n_fft,
                      int hop, int win_length, const float* window, const float* coef,
                      float* g_x, void* ws, size_t ws_bytes, sel_stream_t stream);
/* Finishing arithmetic on device (no host sync): from sums -> out2 = {sc, mag}
 * and, for the backward, coef = {a, b, c, d} (see sel_mag_pair_bwd) given the
 * upstream grads *g_sc, *g_mag (device scalars; NULL = zero).  n = the
 * element count of the log-magnitude mean, or 0: read it from sums[3] (a
 * 4-element sums array whose count was all-reduced on device by a
 * data-parallel caller). */
int sel_stft_loss_finish(const double* sums, int64_t n, float* out2, sel_stream_t stream);
int sel_stft_loss_coef(const double* sums, int64_t n, const float* g_sc, const float* g_mag,
                       float* coef, sel_stream_t stream);

/* ---- log-mel: losses/mel_loss.py:74-94 (MelSpectrogram.forward) -------
 * x (B,T) -> out (B, n_mels, F).  melmat (K, n_mels) is the module buffer;
 * krange (n_mels int2) = nonzero bin range [lo,hi) of each filter, mrange (K int2)
 * = filters touching each bin, both derived from melmat by the host.
 * 0 < n_mels <= n_fft/2 + 12 (SEL_ERR_UNSUPPORTED otherwise, as the backward). */
int sel_logmel_fwd(const float* x, int64_t B, int64_t T, int n_fft, int hop,
                   int win_length, const float* window, const float* melmat,
                   const int32_t* krange, int n_mels, float eps, int log_kind,
                   float* out, sel_stream_t stream);
/* ---- power-mel: mel_spectrogram.py:38-44 (torchaudio MelSpectrogram(48000), eval Mel-L1) --
 * x (B,T) -> out (B, n_mels, F), F = 1 + T/hop: |STFT|^power (center/reflect, periodic
 * window of win_length centred in n_fft, onesided) @ fb (K, n_mels), K = n_fft/2 + 1.
 * n_fft even, n_fft/2 <= 512 with prime factors in {2,3,5} (n_fft 400 -> 200 = 4*2*5*5).
 * krange as for sel_logmel_fwd.  Forward only (an eval metric). */
int sel_power_mel_fwd(const float* x, int64_t B, int64_t T, int n_fft, int hop, int win_length,
                      const float* window, const float* fb, const int32_t* krange, int n_mels, float power,
                      float* out, sel_stream_t stream);
/* L1 between two (n) tensors: losses/mel_loss.py:153 F.l1_loss -> out (1 float, mean). */
size_t sel_l1_workspace(int64_t n);
int sel_l1_mean(const float* a, const float* b, int64_t n, float* out, void* ws,
                size_t ws_bytes, sel_stream_t stream);
/* backward of  g * mean|logmel(x) - ref|  w.r.t. x, or of sum(logmel(x)*g_out) when
 * ref == NULL (then `g_out` (B,M,F) is the upstream gradient, g_scale unused).
 * With ref != NULL: g_out is logmel(x) from the forward and the upstream of each
 * element is (*g_scale) * g_mul * sign(g_out - ref)  (g_mul = 1/N for a mean).
 * Overwrites g_x. */
/* Fused log-mel L1 (mel_loss.py:151-154): *loss = mean |logmel(x) - logmel(y)|
 * over (B, n_mels, F), and, when g_x != NULL, g_x = d loss / d x for a unit
 * upstream (the backward scales it by the upstream gradient): one launch per
 * resolution computes y's and x's log-mels per frame position and x's adjoint
 * (k_mel_l1), then the overlap-add.  mrange / krange as for sel_logmel_bwd.
 * 0 < n_mels <= n_fft/2 + 12.  ws >= sel_mel_l1_workspace(...). */
size_t sel_mel_l1_workspace(int64_t B, int64_t T, int n_fft, int hop, int win_length);
int sel_mel_l1_fwd_grad(const float* x, const float* y, int64_t B, int64_t T, int n_fft, int hop,
                        int win_length, const float* window, const float* melmat, const int32_t* krange,
                        const int32_t* mrange, int n_mels, float eps, int log_kind, float* loss, float* g_x,
                        void* ws, size_t ws_bytes, sel_stream_t stream);
size_t sel_logmel_bwd_workspace(int64_t B, int64_t T, int n_fft, int hop, int win_length);
int sel_logmel_bwd(const float* x, int64_t B, int64_t T, int n_fft, int hop,
                   int win_length, const float* window, const float* melmat,
                   const int32_t* krange, const int32_t* mrange, int n_mels, float eps, int log_kind,
                   const float* g_out, const float* ref, const float* g_scale, float g_mul,
                   float* g_x, void* ws, size_t ws_bytes, sel_stream_t stream);

/* ---- AudioDec conv stack: layers/conv_layer.py, residual_unit.py -------
 * Every conv of the generator is lowered to ONE primitive over channels-last
 * activations (rows = B*T flat, row pitch = channels):
 *   out[m, n] = epi( sum_{k<K} sum_{c<C} Wp[n][k][c] * act(in[row(m,k), c]) )
 *   row(m,k) = b*T + t + k*dil - pad  (t = m % T, b = m / T); rows outside the
 *   sample read 0 (SEL_PAD_ZERO) or clamp to the sample (SEL_PAD_REPLICATE);
 *   act = ELU (alpha 1) when in_elu, else identity;
 *   epi(v) = (v + bias[n % bias_period]) * (aux ? ELU'(aux[m,n]) : 1) + (res ? res[m,n] : 0).
 * Strided convs (encoder down-sampling, conv_layer.py:109-150 with stride s) run
 * as a 3-tap conv on the phase-expanded input (B, T/s, s*Cin); transposed convs
 * (conv_layer.py:153-191) as a 2-tap replicate-padded conv producing
 * (B, T, s*Cout) = (B, T*s, Cout).  Weights are repacked on device each step
 * (sel_pack_weight) and weight gradients unpacked (sel_unpack_wgrad). */
enum { SEL_F32 = 0, SEL_BF16 = 1 };
enum { SEL_PAD_ZERO = 0, SEL_PAD_REPLICATE = 1 };
enum {
  SEL_PACK_FWD = 0,          /* Conv1d W[Cout][Cin][K]          -> Wp[Cout][K][Cin] */
  SEL_PACK_FWD_STRIDED = 1,  /* Conv1d W[Cout][Cin][2s], stride s -> Wp[Cout][3][s*Cin] */
  SEL_PACK_CONVT = 2         /* ConvTranspose1d W[Cin][Cout][2s]  -> Wp[s*Cout][2][Cin] */
};

typedef struct sel_conv_desc {
  int64_t rows;       /* B*T */
  int32_t T;          /* rows per sample */
  int32_t C, N;       /* in / out channels */
  int32_t K, dil, pad;
  int32_t pad_mode;   /* SEL_PAD_* */
  int32_t in_elu;
  int32_t bias_period;/* 0: no bias */
} sel_conv_desc;

/* which kernel instance a bf16 launch uses (for profiling tags); has_epilogue:
 * the launch passes aux and/or res (the thin kernel's epilogue-prefetch variant):
 * ((BM*1000 + BN)*10 + WAVES_M)*10 + KMAX for the tiled kernel,
 * 900000000 + K for the warp-specialised kernel,
 * 1000000000 + E*500000000 + ((R/32*1000 + C)*1000 + N)*10 + K for the
 * weight-stationary thin kernel (E = epilogue-prefetch instance),
 * or -1 for the generic kernel */
int sel_conv_fwd_kernel_id(const sel_conv_desc* d, int in_dtype, int out_dtype, int has_epilogue);
int sel_conv_fwd(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* in,
                 const void* wpack, const float* bias, const void* aux, const void* res,
                 void* out, sel_stream_t stream);
/* Fused residual unit forward (replaces the two sel_conv_fwd calls of
 * models/autoencoder/modules/residual_unit.py:43-46, conv_layer.py:19-23 + :139-142):
 * h = conv1(ELU(x)) [saved for the backward] and out = x + conv1x1(ELU(h)), bf16,
 * C = N in {32, 64} -- or 128 where conv1 alone runs on the (16, 128)
 * k_conv_wss tile (T = 2000-like sequences, >= 65536 rows; sel_tune key 69 = 1
 * turns that off) -- K = 7, causal zero pad; d1 describes conv1 (in_elu = 1).
 * Returns SEL_ERR_UNSUPPORTED for any other shape. */
int sel_resunit_fwd(const sel_conv_desc* d1, int dtype, const void* x, const void* w1pack, const float* b1,
                    const void* w2pack, const float* b2, void* h, void* out, sel_stream_t stream);
/* Fused residual-unit backward at 32 channels (replaces the two adjoint
 * primitive calls of residual_unit.py:43-46's backward): gh = (W2^T g) * ELU'(h),
 * gx = conv1^T(gh) * ELU'(x) + g; d1 is conv1's forward descriptor, wd1/wd2 the
 * dgrad-packed weights (sel_pack_dgrad); gh may be NULL. */
int sel_resunit_bwd(const sel_conv_desc* d1, int dtype, const void* g, const void* h, const void* x,
                    const void* wd1pack, const void* wd2pack, void* gh, void* gx, sel_stream_t stream);
/* The same backward WITH both weight gradients of the unit, in one launch (the
 * residual units whose weights train; 32 channels): gx as sel_resunit_bwd, and
 * per-block fp32 partials of conv1 (part1: nsplit x 32*7*32 packed [N][K][C],
 * then nsplit x 32 bias column sums of gh) and of the 1x1 (part2: nsplit x
 * 32*32, then nsplit x 32 of g).  nsplit = sel_resunit_wgrad_splits(d1, dtype)
 * (a negative code for an unsupported shape); reduce the partials with
 * sel_wgrad_finish_many (kind SEL_PACK_FWD, k 7 and 1). */
int sel_resunit_wgrad_splits(const sel_conv_desc* d1, int dtype);
int sel_resunit_bwd_wgrad(const sel_conv_desc* d1, int dtype, const void* g, const void* h, const void* x,
                          const void* wd1pack, const void* wd2pack, void* gx, float* part1, float* part2,
                          int nsplit, sel_stream_t stream);
/* weight/bias gradient of the same primitive: gwpack[N][K][C] (fp32) and, when
 * gbias != NULL, gbias[bias_period] = sum over rows and phases of gout. */
size_t sel_conv_wgrad_workspace(const sel_conv_desc* d);
int sel_conv_wgrad(const sel_conv_desc* d, int dtype, const void* gout, const void* in,
                   float* gwpack, float* gbias, void* ws, size_t ws_bytes, sel_stream_t stream);
/* sel_conv_wgrad with the weight gradient written straight into the torch layout
 * of the layer's fp32 weight (kind/cout/cin/k/stride as in sel_pack_weight): the
 * unpack is fused into the final reduction pass. */
int sel_conv_wgrad_unpacked(const sel_conv_desc* d, int dtype, const void* gout, const void* in, int kind,
                            int cout, int cin, int k, int stride, float* gw, float* gbias, void* ws,
                            size_t ws_bytes, sel_stream_t stream);
/* Deferred weight gradients (one reduction launch for many layers):
 * sel_conv_wgrad_partials runs only the split-row partial kernel of
 * sel_conv_wgrad into ws (same plan, same partials) and returns the split count
 * in *nsplit; sel_wgrad_finish_many then reduces up to any number of such
 * workspaces in one launch per 24 jobs, with the arithmetic of the per-layer
 * reduction passes (same bits), unpacking into the torch layout (kind >= 0) or
 * writing the packed form (kind < 0).  `jobs` is a HOST array. */
typedef struct sel_wgrad_job {
  const float* part;  /* the workspace of sel_conv_wgrad_partials */
  float* gw;          /* weight gradient (torch layout when kind >= 0) */
  float* gb;          /* bias gradient (bias_period entries) or NULL */
  int64_t nw;         /* N * K * C (packed weight elements) */
  int32_t nsplit, N, bias_period, kind, cout, cin, k, stride;
} sel_wgrad_job;
int sel_conv_wgrad_partials(const sel_conv_desc* d, int dtype, const void* gout, const void* in, int want_bias,
                            void* ws, size_t ws_bytes, int* nsplit, sel_stream_t stream);
int sel_wgrad_finish_many(const sel_wgrad_job* jobs, int njobs, sel_stream_t stream);
/* Repack fp32 torch weights (kind SEL_PACK_*) into Wp (dtype), and the dgrad
 * form of a packed Wp[N][K][C] -> Wd[C][K][N] with taps reversed (the adjoint is
 * the same primitive with pad' = (K-1)*dil - pad). */
int sel_pack_weight(int kind, const float* w, int cout, int cin, int k, int stride,
                    int dtype, void* wpack, sel_stream_t stream);
int sel_pack_dgrad(const void* wpack, int N, int K, int C, int dtype, void* wd,
                   sel_stream_t stream);
/* Batched form of sel_pack_weight + sel_pack_dgrad for many layers in one launch.
 * `jobs` is a DEVICE array of njobs entries sorted by `offset` (the prefix sum of
 * each job's packed element count); total = sum of the counts.  wdgrad may be NULL. */
typedef struct sel_pack_job {
  const float* w;     /* torch-layout fp32 weight */
  void* wpack;        /* Wp (dtype) */
  void* wdgrad;       /* dgrad form of Wp (dtype) or NULL */
  int64_t offset;
  int32_t kind, cout, cin, k, stride, reserved;
} sel_pack_job;
int sel_pack_many(const sel_pack_job* jobs, int njobs, int64_t total, int dtype, sel_stream_t stream);
/* The same with `jobs` in HOST memory (copied into the kernel arguments, 48
 * jobs per launch; offsets increasing): no device job table to stage.  The
 * product path (sel.convops.PackCache) uses this one. */
int sel_pack_many_host(const sel_pack_job* jobs, int njobs, int64_t total, int dtype, sel_stream_t stream);
/* gwpack (packed fp32) -> torch layout gw (kind as in sel_pack_weight). */
int sel_unpack_wgrad(int kind, const float* gwpack, int cout, int cin, int k, int stride,
                     float* gw, sel_stream_t stream);
/* adjoint of SEL_PAD_REPLICATE (pad 1, K 2): gin[b*T + 0, c] += sum_n gout[b*T + 0, n] * Wp[n][0][c] */
int sel_conv_replicate_fix(const sel_conv_desc* d, int dtype, const void* gout,
                           const void* wpack, void* gin, sel_stream_t stream);
/* dtype casts (activations in/out of the bf16 path) */
int sel_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n,
             sel_stream_t stream);

/* ---- streaming step: layers/conv_layer.py:144-147 (CausalConv1d.inference),
 * :185-188 (CausalConvTranspose1d.inference), residual_unit.py:78-81 ---------
 * One causal layer of one streaming hop, on channels-last rows, with the
 * reference's pad_buffer as an explicit carry.  Same descriptor as sel_conv_fwd:
 *   T = d->T NEW rows per sample, B = d->rows / T, P = (K-1)*dil;
 *   d->pad must equal P and pad_mode must be SEL_PAD_ZERO (SEL_ERR_ARG otherwise);
 *   v[b] = [ carry[b] (P rows) | act(in[b]) (T rows) ], act = ELU when in_elu,
 *          applied to the new rows only (the carry holds what pad_buffer holds:
 *          for a residual unit's conv1 the ACTIVATED signal);
 *   out[b,t,n] = sum_{k,c} Wp[n][k][c] * v[b, t + k*dil, c] + bias[n % bias_period] + res[b,t,n];
 *   carry_out[b] = the last P rows of v[b], in in_dtype, copied bit for bit
 *          (T < P keeps P - T rows of the old carry).  carry is never written;
 *          carry_out must not alias carry (SEL_ERR_ARG).  K = 1: P = 0, carry and
 *          carry_out may be NULL (the residual unit's 1x1 with its + x as res).
 * Wp is what sel_pack_weight writes: SEL_PACK_FWD as is; SEL_PACK_FWD_STRIDED a
 * 3-tap conv over the phase view (C = s*Cin, P = 2 phase rows = 2s samples, the
 * oldest of which meets a structurally zero weight); SEL_PACK_CONVT a 2-tap conv
 * with N = s*Cout and P = 1 (the previous input row where the training forward
 * replicates), out viewed as (T*s, Cout) = deconv(cat(buf, x))[s:-s].
 * in_dtype / out_dtype: fp32 -> fp32, bf16 -> bf16 or fp32; res has the output
 * type.  Any C and N; C % 8 == 0 with 16-byte aligned pointers takes 16-byte
 * operand loads.  The K*C reduction is split over the waves of a block by the
 * layer shape alone and summed in wave order: no atomics, two calls give the
 * same bits, and a sample's output does not depend on B or T.  No workspace.
 * Arguments are validated before any device work. */
int sel_conv_step(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* carry, const void* in,
                  const void* wpack, const float* bias, const void* res, void* out, void* carry_out,
                  sel_stream_t stream);
/* End of a hop: copy every layer's carry_out into its carry in one launch per
 * 48 jobs (`jobs` is a HOST array, copied into the kernel arguments), so all
 * streaming state lives at fixed addresses and a hop can be captured in a graph. */
typedef struct sel_copy_job {
  const void* src;
  void* dst;
  int64_t bytes;
} sel_copy_job;
int sel_stream_commit(const sel_copy_job* jobs, int njobs, sel_stream_t stream);

/* ---- stream pools: independent streams on slot-indexed steps ----------------
 * sel_conv_step with a slot table: one batched step over whichever streams have
 * a hop ready on this tick.  d->rows = capacity * T sizes the launch (grid, the
 * RT switch) and never changes; the wave count depends on K*C alone.
 *   slots     DEVICE int32[>= capacity], n_active DEVICE int32 (both required);
 *   n = min(*n_active, capacity) samples exist on this tick (negative: 0);
 *   sample i reads its T new rows at in[i*T ..] (res likewise) and writes
 *          out[i*T ..]: in / res / out are DENSE in active order;
 *   sample i reads its P carried rows at carry[slots[i]] and writes
 *          carry_out[slots[i]]: both are pools of nslots (> 0) slot rows of pitch
 *          P*C elements, in in_dtype.
 * Row groups that lie entirely at or beyond n*T return before any load (conv
 * blocks and carry-writer blocks alike); nothing is written for rows >= n*T of
 * out nor for a slot that is not in the list.  A list entry outside [0, nslots)
 * makes that sample absent -- nothing is read through it, nothing is written for
 * it: a guard, not a feature.  Entries must be distinct (two samples on one
 * slot race on carry_out; sel.streamops.SlotTable enforces it).
 * Everything else is sel_conv_step's and validated before any device work: the
 * dtypes, the aliasing rules, K = 1 with NULL pools, the pack kinds, the 16-byte
 * fast path (C % 8 == 0, aligned in / wpack / carry).  The output rows and the
 * carry_out row of sample i are, bit for bit, what sel_conv_step gives at B = 1
 * on that slot's carry and those input rows. */
int sel_conv_step_pool(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* carry, void* carry_out,
                       int nslots, const int32_t* slots, const int32_t* n_active, const void* in, const void* wpack,
                       const float* bias, const void* res, void* out, sel_stream_t stream);
/* Slot rows between pools: for i < min(*n, cap) and every job, slot row
 * src_slots[i] of job.src -> slot row dst_slots[i] of job.dst, where job.bytes
 * is the pitch of one slot row and both pools hold nslots rows.  `jobs` is a
 * HOST array (copied into the kernel arguments, 48 per launch); src_slots,
 * dst_slots (DEVICE int32[>= cap]) and n (DEVICE int32) are read by the kernel,
 * so one captured launch serves every tick.  16-byte vectors where both rows
 * are 16-byte aligned, then a byte tail; an entry outside [0, nslots) skips its
 * row.  Two uses: the commit of a pool hop (carry_out -> carry with src_slots =
 * dst_slots = the tick's list) and opening a stream (the template row of every
 * carry -> the new slot; src and dst may then be the same pool -- rows must not
 * overlap, i.e. no dst_slots entry equals a src_slots entry of another i). */
int sel_stream_copy_slots(const sel_copy_job* jobs, int njobs, int nslots, const int32_t* src_slots,
                          const int32_t* dst_slots, int cap, const int32_t* n, sel_stream_t stream);

/* ---- residual VQ: layers/vq_module.py:61-88 (eval), :119-134 -------------
 * All stages of one row block in one launch (rows are independent):
 *   dist_k = (|r|^2 - (2r).e_k) + |e_k|^2, idx = argmin (lowest index on ties),
 *   q = e_idx, qst = r + (q - r), r <- r - qst, out += qst.
 * x (N, D) fp32; embeds (S, D, K) fp32 (the `embed` buffers stacked);
 * out (N, D); idx (S, N) int64; counts (S, K) int32 (zeroed by the call);
 * sqerr (S) fp64: sum (q - r)^2 per stage. */
size_t sel_rvq_workspace(int64_t N, int S, int K);
int sel_rvq_fwd(const float* x, int64_t N, int D, const float* embeds, int S, int K,
                float* out, int64_t* idx, int32_t* counts, double* sqerr,
                void* ws, size_t ws_bytes, sel_stream_t stream);
/* per-stage loss = sqerr/(N*D)*commitment and perplexity from counts -> loss[S], ppl[S] */
int sel_rvq_finish(const int32_t* counts, const double* sqerr, int64_t N, int D, int S, int K,
                   float commitment, float* loss, float* ppl, sel_stream_t stream);
/* g_x = g_out + g_loss[0]*commitment*2*(x - e0[idx0])/(N*D)  (only stage 0's
 * commitment term reaches x: later residuals have zero Jacobian w.r.t. x, vq_module.py:83,129) */
int sel_rvq_bwd(const float* x, int64_t N, int D, const float* embed0, int K, const int64_t* idx0,
                const float* g_out, const float* g_loss, float commitment, float* g_x,
                sel_stream_t stream);

/* ---- residual VQ for a streaming hop: the quantizer and the lookup as step
 * launches (csrc/vq_step.hip) --------------------------------------------------
 * Both calls only enqueue one kernel: no allocation, no workspace, no host
 * synchronisation, no prep launch, no state -- they can be captured in a graph
 * behind / in front of the conv steps of a hop.  Arguments are validated before
 * any device work (SEL_ERR_ARG).
 *
 * Active set (both): rows = B * rows_per_sample.  n_active NULL: every row is
 * active.  Otherwise n_active is a DEVICE int32 and n = clamp(*n_active, 0, B);
 * rows >= n * rows_per_sample are neither read nor written, and a block that
 * lies entirely beyond them returns after reading the count (as the pool step
 * kernels do).  There is no slot list: in and out are dense in active order.
 *
 * sel_rvq_step: z (rows, D) fp32 -> idx (S, rows) int64 and, unless zq is NULL,
 * zq (rows, D) fp32.  embeds (S, D, K) fp32, the `embed` buffers stacked.  Per
 * (row, stage, code) the arithmetic is sel_rvq_fwd's direct kernel exactly:
 *   |r|^2: lanes over d (d = lane, lane + 64, ...), fmaf, then the wave's xor butterfly;
 *   dot_k and |e_k|^2: fmaf chains over d ascending from 0, on the same loaded values;
 *   dist_k = (|r|^2 - 2 dot_k) + |e_k|^2, idx = argmin, lowest index on ties;
 *   q = e_idx, qst = r + (q - r), r <- r - qst, zq += qst (zq starts at 0).
 * For finite z, idx (before the offset) and zq are bit for bit what sel_rvq_fwd
 * writes under every setting of tune keys 2 and 39.  flatten != 0 adds s*K to
 * stage s's picks (ResidualVQ.forward_index(flatten_idx=True): ids into the flat
 * codebook).  The pick is forced into [0, K) before the gather: a row whose
 * distances are all NaN picks code 0 and reads nothing outside the stack.
 * One workgroup per row, threads over codes; a row's bits depend on that row
 * alone.  D = 64 with K = 1024 takes a register-resident instance, everything
 * else a generic loop with the same arithmetic.
 * Accepted: rows >= 1, rows % rows_per_sample == 0, 0 < D <= 256, K > 0, S > 0
 * (no upper limit on S: idx is written per stage); z, embeds, idx non-null; zq
 * must not alias z.
 *
 * sel_rvq_lookup_step: idx (S, rows) int64, ids into codebook (ncodes, D) fp32
 * (ResidualVQ.initial()'s flat layout, ncodes = S*K there) -> out (rows, D):
 *   acc = codebook[idx[0,row]]; acc = acc + codebook[idx[s,row]] for s = 1 .. S-1
 *   in that order, each a round-to-nearest fp32 add;
 *   with mean / scale (D floats each, both or neither): acc = (acc - mean[d]) / scale[d],
 *   a correctly rounded subtraction and division (HiFiGAN decode_norm);
 *   stored as fp32, or as bf16 rounded to nearest even (out_dtype).
 * An id outside [0, ncodes) contributes zero and nothing is read through it.
 * 16-byte vectors where D % 4 == 0 and codebook / out / mean / scale are
 * 16-byte aligned, element-wise otherwise (same bits).
 * Accepted: rows >= 1, rows % rows_per_sample == 0, S > 0, D > 0, ncodes > 0;
 * idx, codebook, out non-null. */
int sel_rvq_step(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                 const int32_t* n_active, int flatten, int64_t* idx, float* zq, sel_stream_t stream);
int sel_rvq_lookup_step(const int64_t* idx, int rows, int rows_per_sample, int S, int64_t ncodes, int D,
                        const float* codebook, const float* mean, const float* scale, const int32_t* n_active,
                        int out_dtype, void* out, sel_stream_t stream);

/* ---- the wire format of the code indices, version 1 (csrc/vq_step.hip, sel/wire.py) ----
 * What a transmitter sends per hop: the picks of sel_rvq_step, bit-packed.
 *   bits        = max(1, ceil(log2 K)): the width of one field.
 *   record      one per row: the S un-flattened codes k_s in [0, K), field s in bits
 *               [s*bits, (s+1)*bits) of the record read as a little-endian bit
 *               string -- bit i of the record is bit i % 8 of byte i / 8.
 *   frame_bytes = ceil(S*bits / 8).  The pad bits of the last byte are written as
 *               zero and ignored on reading.
 *   packet      a stream's `frames` records of one hop back to back:
 *               packet_bytes = frames * frame_bytes.  A wire buffer is a dense
 *               (rows, frame_bytes) uint8 array in row order.
 * Every row owns its bytes: no byte is shared between rows, so no two blocks write
 * the same byte and nothing is atomic.  S = 8, K = 1024: 10 bytes per frame (at 160
 * frames/s, 12.8 kbit/s).  There is no header, no sequence number and no checksum.
 *
 * Both calls below are single launches with the contract of their siblings above:
 * no workspace, no allocation, no host synchronisation, capturable, the same
 * active set (rows >= n * rows_per_sample: neither read nor written, wire bytes
 * included), arguments validated before any device work (SEL_ERR_ARG).
 *
 * sel_rvq_step_wire: sel_rvq_step with the rows' records written by the same
 * launch.  The picks, idx and zq are bit for bit sel_rvq_step's (one kernel body,
 * instantiated with and without the record).  The first wave shifts each stage's
 * pick into a 64-bit accumulator and stores the bytes that fill, so S stays
 * unbounded; the last partial byte is stored zero-padded.  Byte stores only: wire
 * may have any alignment.  idx may be NULL here (zq as before); wire must not be.
 * Accepted: what sel_rvq_step accepts (idx apart), bits <= 31, S*K <= 2^40.
 *
 * sel_rvq_lookup_wire_step: sel_rvq_lookup_step on the ids s*K + k_s taken out of
 * the records, with no int64 buffer in between; codebook is (S*K, D).  Same
 * ascending round-to-nearest adds, same mean / scale step, same fp32 / bf16 store,
 * same 16-byte path with an element-wise fallback (one kernel body again).
 * Packets come off a network: a field >= K contributes zero and nothing is read
 * through it; pad bits are ignored; wire is read byte by byte, never beyond a
 * row's own frame_bytes, and may have any alignment.  idx_out (S, rows) int64,
 * when non-null, receives the flattened ids, -1 for a refused field.
 * Accepted: what sel_rvq_lookup_step accepts with ncodes = S*K (wire for idx),
 * K > 0, bits <= 31, S*K <= 2^40. */
#define SEL_WIRE_VERSION 1
int sel_rvq_step_wire(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                      const int32_t* n_active, int flatten, int64_t* idx, float* zq, uint8_t* wire,
                      sel_stream_t stream);
int sel_rvq_lookup_wire_step(const uint8_t* wire, int rows, int rows_per_sample, int S, int K, int D,
                             const float* codebook, const float* mean, const float* scale, const int32_t* n_active,
                             int out_dtype, void* out, int64_t* idx_out, sel_stream_t stream);

/* ---- the datagram, wire version 2 (csrc/vq_step.hip, sel/wire.py) ----
 * What a sender puts on a network per hop and stream: a header and the hop's
 * records truncated to the s <= S stages the sender chose (a residual VQ is a
 * scalable code: the first s stages are a coarser code of the same frame).
 *   byte 0      2                          the version
 *   byte 1      s, 1 <= s <= S             stages carried by this datagram
 *   bytes 2..3  seq, uint16 little-endian  the hop number of the stream, wrapping
 *   bytes 4..   `frames` records: version 1's record with S replaced by s --
 *               field j < s in bits [j*bits, (j+1)*bits), fb(s) = ceil(s*bits / 8)
 *               bytes, pad bits written as zero and ignored on reading.
 * A datagram is 4 + frames * fb(s) bytes; `frames` is not in the header (a
 * receiver knows its own).  S <= 255.  S = 8, K = 1024: fb(1..8) = 2, 3, 4, 5, 7,
 * 8, 9, 10.  A datagram buffer is (B, dgram_stride) uint8 with dgram_stride >=
 * 4 + frames * fb(S): sample i owns [i*dgram_stride, (i+1)*dgram_stride), of
 * which only the first 4 + frames * fb(s_i) bytes are written by the transmitter
 * or read by the receiver.  No byte is shared between samples, nothing is
 * atomic, byte accesses only: any start address and any stride.
 *
 * Both calls are single launches with their siblings' contract (no workspace,
 * no allocation, no host synchronisation, capturable, SEL_ERR_ARG before any
 * device work) and their active set: rows >= n * rows_per_sample are neither
 * read nor written -- datagram bytes, idx, zq, out, idx_out and hold rows
 * included.  stages, seq, slots and lost are DEVICE int32 arrays, dense in
 * active order, one entry per sample i = row / rows_per_sample, so one captured
 * launch serves every mix of budgets and losses staged into them.
 *
 * sel_rvq_step_dgram: s_i = clamp(stages[i], 1, S) (stages NULL: S; seq NULL: 0).
 * A row's block runs sel_rvq_step's chain for stages 0 .. s_i - 1 and stops; the
 * later codebooks are not requested.  Those picks are bit for bit the first s_i
 * picks of sel_rvq_step on the row, zq is sel_rvq_step's with S = s_i on
 * embeds[:s_i], idx[s, row] = -1 for s >= s_i (idx may be NULL).  The row's
 * record of s_i fields goes to dgram + i*dgram_stride + 4 + r*fb(s_i), r = row %
 * rows_per_sample; the block of the sample's first row writes the header, seq[i]
 * as its low 16 bits.  Bytes beyond the datagram's length are not written.
 * Accepted: what sel_rvq_step_wire accepts, S <= 255, dgram non-null,
 * dgram_stride >= 4 + rows_per_sample * fb(S).
 *
 * sel_rvq_lookup_dgram_step: sample i is valid when lost is NULL or lost[i] == 0,
 * byte 0 of its datagram is 2 and byte 1 is in [1, S]; a bad header makes the
 * sample lost and nothing is read outside its region or the codebook.  slot =
 * slots ? slots[i] : i; hold is (nslots, hold_stride) uint8, a row being {stages
 * held (0: none), that record}.
 *   valid: every row sums the fields of its own record as
 *     sel_rvq_lookup_wire_step does (k >= K refused, pad bits ignored) -- bit for
 *     bit sel_rvq_lookup_step on ids j*K + k_j for j < s_i and -1 beyond -- and
 *     the sample's LAST row's record and s_i are copied into hold[slot];
 *   lost: every row of the sample sums the record held by its slot, hold is not
 *     written; nothing held (count 0, hold NULL, slot outside [0, nslots)) is
 *     the empty sum, +0.0f per channel, then mean / scale.
 * Within a launch a sample reads its hold row or writes it, never both; the
 * slots of a launch must be distinct.  idx_out (S, rows), when non-null, receives
 * the ids summed: the held ones on a lost hop, -1 for refused or absent fields.
 * Accepted: what sel_rvq_lookup_wire_step accepts, S <= 255, the stride bound
 * above, hold NULL or hold_stride >= 1 + fb(S) with nslots >= 1. */
#define SEL_DGRAM_VERSION 2
#define SEL_DGRAM_HEADER_BYTES 4
int sel_rvq_step_dgram(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                       const int32_t* n_active, const int32_t* stages, const int32_t* seq, int flatten,
                       int64_t* idx, float* zq, uint8_t* dgram, int64_t dgram_stride, sel_stream_t stream);
int sel_rvq_lookup_dgram_step(const uint8_t* dgram, int64_t dgram_stride, int rows, int rows_per_sample,
                              int S, int K, int D, const float* codebook, const float* mean, const float* scale,
                              const int32_t* n_active, const int32_t* slots, const int32_t* lost,
                              uint8_t* hold, int64_t hold_stride, int nslots,
                              int out_dtype, void* out, int64_t* idx_out, sel_stream_t stream);

/* ---- residual VQ, training mode: the EMA codebook update, vq_module.py:74-80 ----
 * Runs after sel_rvq_fwd on the same x / embeds / idx / counts.  Training mode
 * changes nothing about the assignment (every stage picks its code with its own
 * pre-update codebook), so this call is only the update, for all stages at once.
 *
 * Contract:
 *   r_0 = x, r_{s+1} = r_s - (r_s + (e_s[idx_s] - r_s)): the forward's three fp32
 *   operations in that order, so the residuals are the bits the forward used.
 *   sum_s[d][k] = sum over {n : idx[s,n] = k} of r_s[n][d], in fp32, rows added in
 *   ascending n: the order is fixed by idx alone.  No float atomics; two calls
 *   on the same inputs give the same bits.
 *   For each stage with update != 0 (omd = 1 - decay in fp32):
 *     cluster_size <- cluster_size*decay + counts*omd
 *     n  = sum_k cluster_size   (fixed-order reduction accumulated in double)
 *     cs = (cluster_size + eps) / (n + K*eps) * n
 *     embed_avg <- embed_avg*decay + sum*omd
 *     embed <- embed_avg / cs
 *   A code with no rows decays like any other (the same formula, zero sum).
 *   Stages with update == 0 are in eval mode: their three buffers are not written.
 * `embeds` (S, D, K) is the stack the forward read; it is read-only here (the
 * backward reads it after the update) and must not alias any stage's `embed`.
 * `counts` (S, K) must be the histogram of `idx` (S, N), as sel_rvq_fwd leaves it.
 * The per-stage table is in HOST memory and is copied into the kernel arguments
 * (as sel_pack_many_host's jobs): the modules keep one buffer per layer.
 * The call enqueues on `stream`, makes no host synchronisation and no allocation,
 * and can be captured into a graph.  Arguments are validated before any device
 * work: N >= 1 (N == 0 is refused, as sel_rvq_finish refuses it), 0 < D <= 256,
 * 0 < S <= 16, K > 0 (SEL_ERR_ARG); ws_bytes >= sel_rvq_ema_workspace
 * (SEL_ERR_WORKSPACE); non-null pointers (SEL_ERR_ARG). */
typedef struct sel_rvq_ema_stage {   /* one per stage, host memory, copied into the kernel arguments */
  float* embed;         /* (D, K) in/out  */
  float* cluster_size;  /* (K)    in/out  */
  float* embed_avg;     /* (D, K) in/out  */
  int32_t update;       /* 0: stage is in eval mode, its three buffers are not written */
  int32_t reserved;
} sel_rvq_ema_stage;
size_t sel_rvq_ema_workspace(int64_t N, int D, int S, int K);
int sel_rvq_ema_update(const float* x, int64_t N, int D, const float* embeds /* (S,D,K): the stack the forward read */,
                       int S, int K, const int64_t* idx /* (S,N) */, const int32_t* counts /* (S,K) */,
                       const sel_rvq_ema_stage* stages, float decay, float eps,
                       void* ws, size_t ws_bytes, sel_stream_t stream);

/* ---- the same update in two halves, for data-parallel training: vq_module.py:74-80 ----
 * sel_rvq_ema_update folds each code's sum straight into embed_avg, so its
 * statistics never exist on their own.  This pair stops in between: the stats
 * call leaves the per-code sums and counts of this rank's rows in a buffer the
 * ranks exchange (sel.dist.gather_blocks: gathered in rank order, not
 * all-reduced), the apply call folds the gathered blocks into the codebooks.
 * sel_rvq_ema_update itself is unchanged.
 *
 * Contract of sel_rvq_ema_stats (after sel_rvq_fwd on the same x / embeds / idx):
 *   r_s as above: the forward's three fp32 operations in its order.
 *   Segment g (0 <= g < nseg) is the rows [g*N/nseg, (g+1)*N/nseg).
 *   stats is (nseg, S, D+1, K) fp32, sel_rvq_ema_stats_floats(D,S,K) = S*(D+1)*K
 *   floats per block.  Block g, stage s:
 *     planes 0..D-1: sum[d][k] = sum over {n in segment g : idx[s,n] = k} of
 *                    r_s[n][d], in fp32 from 0, rows added in ascending n;
 *     plane D:       the number of those rows, as fp32 (exact: a segment has at
 *                    most 2^24 rows).
 *   EVERY element of stats is written, codes without rows included (zeros): the
 *   caller need not clear it.  No float atomics; two calls on the same inputs
 *   give the same bits.
 *   Validated before any device work: the shape limits of sel_rvq_ema_update;
 *   1 <= nseg <= 65535, N % nseg == 0, N/nseg <= 2^24 (SEL_ERR_ARG);
 *   ws_bytes >= sel_rvq_ema_stats_workspace (SEL_ERR_WORKSPACE); non-null
 *   pointers (SEL_ERR_ARG).
 *
 * Contract of sel_rvq_ema_apply on stats (nblk, S, D+1, K), nblk >= 1 blocks of
 * that layout (nblk = ranks x segments per rank, in rank-major order).  For each
 * stage with update != 0 (omd = 1 - decay in fp32):
 *     sum = ((blk_0 + blk_1) + blk_2) + ...       fp32, left to right in block order
 *     cnt = blk_0 + blk_1 + ...                   the count plane, in double,
 *                                                 converted to float once
 *     embed_avg    <- fmaf(sum, omd, embed_avg*decay)
 *     cluster_size <- fmaf(float(cnt), omd, cluster_size*decay)
 *     n, cs, embed as in sel_rvq_ema_update (the same fixed fp64 tree for n).
 *   Stages with update == 0 are not written.  The result depends on the blocks
 *   and their order alone, so every rank that applies the same gathered blocks
 *   to equal codebooks keeps equal codebooks, for any number of ranks, whatever
 *   the collective's algorithm.  With nseg = nblk = 1 the pair writes the bits
 *   of sel_rvq_ema_update.
 *   The stage table is in HOST memory, as above.  Validated before any device
 *   work: 0 < D <= 256, 0 < S <= 16, K > 0, nblk >= 1, non-null stats / table,
 *   non-null buffers in every stage with update != 0 (all SEL_ERR_ARG).
 * Both calls enqueue on `stream`, make no host synchronisation and no
 * allocation, and can be captured into a graph. */
size_t sel_rvq_ema_stats_floats(int D, int S, int K);
size_t sel_rvq_ema_stats_workspace(int64_t N, int D, int S, int K);
int sel_rvq_ema_stats(const float* x, int64_t N, int D, const float* embeds /* (S,D,K): the stack the forward read */,
                      int S, int K, const int64_t* idx /* (S,N) */, int nseg,
                      float* stats /* (nseg, S, D+1, K) */, void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_rvq_ema_apply(const float* stats /* (nblk, S, D+1, K) */, int nblk, int D, int S, int K,
                      const sel_rvq_ema_stage* stages, float decay, float eps, sel_stream_t stream);

/* ---- data glue: dataloader/data_utils.py:12-22 (add_noise) ---------------
 * out = (exp(snr/10) * ||noise||_2 / ||speech||_2 * speech + noise) / 2 with
 * BATCH-GLOBAL norms over all n elements (math.exp, not 10^x, as the reference). */
size_t sel_add_noise_workspace(int64_t n);
int sel_add_noise(const float* speech, const float* noise, int64_t n, float snr, float* out,
                  void* ws, size_t ws_bytes, sel_stream_t stream);
/* the same in two halves for data-parallel mixing: per-rank sums2 = {sum s^2, sum n^2}
 * (device doubles, all-reduced by the caller across ranks), then the mix */
int sel_sumsq2(const float* speech, const float* noise, int64_t n, double* sums2, void* ws,
               size_t ws_bytes, sel_stream_t stream);
int sel_mix_noise(const float* speech, const float* noise, int64_t n, const double* sums2, float snr,
                  float* out, sel_stream_t stream);

/* ---- BatchNorm1d (models/autoencoder/modules/projector.py:40-44, model='conv1d_bn';
 * replaces torch.nn.BatchNorm1d.forward / its autograd backward) -------------
 * x, y, gy, gx: (rows, C) fp32 channels-last (rows = B*T).  training: batch
 * statistics (biased variance for the normalisation; running_mean / running_var,
 * when given, updated with `momentum` and the unbiased variance, as torch);
 * otherwise the running statistics.  save_mean / save_invstd (C floats) are
 * written by the forward and read by the backward.  gamma / beta may be null
 * (affine=False); ggamma / gbeta / gx may be null (not wanted).  ws: at least
 * sel_batchnorm_workspace(rows, C) bytes. */
size_t sel_batchnorm_workspace(int64_t rows, int C);
int sel_batchnorm_fwd(const float* x, int64_t rows, int C, const float* gamma, const float* beta, int training,
                      float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                      float* save_invstd, float* y, void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_batchnorm_bwd(const float* x, const float* gy, int64_t rows, int C, const float* gamma,
                      const float* save_mean, const float* save_invstd, int training, float* gx, float* ggamma,
                      float* gbeta, void* ws, size_t ws_bytes, sel_stream_t stream);

/* ---- optimizer step (trainer/trainerGAN.py:271-281 optimizer.step()) ---- */
/* Adam update (torch.optim.Adam semantics: L2 weight decay, no amsgrad /
 * maximize) of nt fp32 tensors in one launch: per element, g += wd p;
 * m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
 * p -= step_size m / (sqrt(v) / bc2_sqrt + eps), step_size = lr / (1 - b1^t),
 * bc2_sqrt = sqrt(1 - b2^t) (computed by the caller from the step count t). */
typedef struct {
  float* p;
  const float* g;
  float* m;  /* exp_avg */
  float* v;  /* exp_avg_sq */
  int64_t n;
} sel_adam_tensor;
int sel_adam_step_many(const sel_adam_tensor* ts, int nt, double beta1, double beta2, double eps,
                       double weight_decay, double step_size, double bc2_sqrt, sel_stream_t stream);
/* The same update with the step count and learning rate on the device (the
 * capturable form: a HIP-graph replay of a training step stays correct, the
 * role of torch.optim.Adam(capturable=True)): *step += 1, then step_size =
 * lr[0] / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t) computed in double on the
 * device into consts[0..1] (caller-owned, 2 floats), then the update.  One
 * step count for all nt tensors (one parameter group). */
int sel_adam_step_many_dev(const sel_adam_tensor* ts, int nt, double beta1, double beta2, double eps,
                           double weight_decay, const float* lr, float* step, float* consts,
                           sel_stream_t stream);

/* ---- SNR term of train_denoise.py:140 (torchmetrics 1.2.0 SignalNoiseRatio,
 * zero_mean=False): snr_b = 10 log10((sum t^2 + eps) / (sum (t-p)^2 + eps)) over the
 * last dim, out[0] = mean_b snr_b.  bwd: g_p = g * 20/ln10 * (t-p) / (D_b + eps) / B. */
int sel_snr_fwd(const float* pred, const float* target, int64_t B, int64_t T, double* sums /*2B*/,
                float* out, sel_stream_t stream);
int sel_snr_bwd(const float* pred, const float* target, int64_t B, int64_t T, const double* sums,
                const float* g_out, float* g_pred, sel_stream_t stream);

/* ---- evaluation measures (the reference's mel_spectrogram.py:47-64) ----
 * Every call below refuses bad arguments before any device work (null
 * pointers, B or T <= 0, flags outside {0, 1}: SEL_ERR_ARG; a short workspace:
 * SEL_ERR_WORKSPACE), enqueues on `stream`, allocates nothing, makes no host
 * synchronisation and can be captured into a graph.  ws: caller-owned, 8-byte
 * aligned, at least the matching *_workspace bytes.
 *
 * SDR family over the last dim of (B, T) fp32, eps = FLT_EPSILON, row sums in
 * fp64; with zero_mean each row's mean is subtracted from both signals first.
 *   scale_invariant = 0: 10 log10((sum t^2 + eps) / (sum (t - p)^2 + eps))
 *   scale_invariant = 1 (torchmetrics 1.2.0 scale_invariant_signal_distortion_ratio):
 *     alpha = (sum p t + eps) / (sum t^2 + eps), ts = alpha t,
 *     10 log10((sum ts^2 + eps) / (sum (ts - p)^2 + eps))
 * fwd writes vals (B) and mean (1) and leaves the row sums in ws for bwd.
 * bwd: g_pred (B, T) = d(sum_b g_vals[b] vals[b] + g_mean[0] mean) / d pred;
 * either of g_vals (B) / g_mean (1) may be null, not both.
 * (scale_invariant = 0, zero_mean = 0) runs sel_snr_fwd / sel_snr_bwd: mean
 * and (with g_vals null) g_pred are theirs bit for bit. */
size_t sel_sdr_workspace(int64_t B);
int sel_sdr_fwd(const float* pred, const float* target, int64_t B, int64_t T, int scale_invariant, int zero_mean,
                float* vals /*B*/, float* mean /*1*/, void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_sdr_bwd(const float* pred, const float* target, int64_t B, int64_t T, int scale_invariant, int zero_mean,
                const float* g_vals /*B, may be NULL*/, const float* g_mean /*1, may be NULL*/, float* g_pred,
                const void* ws, size_t ws_bytes, sel_stream_t stream);
/* STOI (extended = 0) / ESTOI (extended = 1) of (B, T) fp32 signals at 10 kHz,
 * T >= 256, B <= 65535: frame 256, hop 128, Hann(258)[1:-1], frames of the
 * clean signal more than 40 dB below its loudest dropped from both, 512-point
 * FFT, 15 third-octave bands from 150 Hz, segments of 30 frames.
 * d (B); mean (1, may be NULL); info (int32 3 B, may be NULL): frames, frames
 * kept, M = kept - 1 re-framed columns, per row.  A row with M < 30 gets 1e-5.
 * sel_stoi_band_edges: band b sums bins [edges[b], edges[b + 1]) (16 ints, host). */
size_t sel_stoi_workspace(int64_t B, int64_t T);
int sel_stoi(const float* clean, const float* proc, int64_t B, int64_t T, int extended, float* d /*B*/,
             float* mean /*1, may be NULL*/, int* info /*3B, may be NULL*/, void* ws, size_t ws_bytes,
             sel_stream_t stream);
int sel_stoi_band_edges(int* edges /*16*/);
/* Gradient of STOI / ESTOI with respect to the processed signal;
 * the clean signal is data.  g_proc (B, T) = d(sum_b g_d[b] d[b] + g_mean[0]
 * mean) / d proc, i.e. row b is scaled by g_row = g_d[b] + g_mean[0] / B; either
 * of g_d (B) / g_mean (1) may be null, not both.  ws_fwd is the workspace that
 * sel_stoi filled for the same (clean, proc, B, T): the kept-frame lists, the
 * counts and the band magnitudes are read from it and it is not written.
 * ws_bwd: sel_stoi_bwd_workspace(B, T) bytes, 8-byte aligned like ws_fwd.
 * The silent-frame mask is a constant selection (no gradient flows through it).
 * The STOI clip min(c y, beta x) takes the c y branch (c depends on y) where
 * c y < beta x and is a constant otherwise (c still depends on y in the other
 * cells of that band).  Exactly 0: the cells of a band magnitude that is exactly
 * 0; every sample of a row with M < 30 (its d is the constant 1e-5); samples
 * that no kept frame covers; the tail past the last frame.  Every element of
 * g_proc is written by the call.  fp64 inside, no atomics: the same bits run
 * to run.  Refusals as sel_stoi, plus a null g_proc, g_d and g_mean both null
 * and a workspace that is not 8-byte aligned (SEL_ERR_ARG). */
size_t sel_stoi_bwd_workspace(int64_t B, int64_t T);
int sel_stoi_bwd(const float* clean, const float* proc, int64_t B, int64_t T, int extended,
                 const float* g_d /*B, may be NULL*/, const float* g_mean /*1, may be NULL*/, float* g_proc /*(B, T)*/,
                 const void* ws_fwd, size_t ws_fwd_bytes, void* ws_bwd, size_t ws_bwd_bytes, sel_stream_t stream);
/* BSS-eval SDR: torchmetrics 1.2.0 signal_distortion_ratio with the
 * direct solve, over the last dim of (B, T) fp32, L = filter_length in [1, 512],
 * B <= 65535, T <= 2^32.  In fp64: subtract each row's mean (zero_mean),
 * t /= max(||t||, 1e-6), p /= max(||p||, 1e-6), r[k] = sum_n t[n] t[n + k] and
 * b[k] = sum_n t[n] p[n + k] for k < L (LINEAR correlations: terms with
 * n + k >= T are absent, lags k >= T are 0; torchmetrics' wrapped lags at T < L
 * are not reproduced), r[0] += load_diag (0: none; negative or not finite:
 * SEL_ERR_ARG), sol = toeplitz(r)^-1 b (Levinson recursion), coh = b . sol,
 * vals[row] = 10 log10(coh / (1 - coh)).  1 - coh <= 0 gives +inf; a silent
 * target (r[0] <= 0) gives NaN in that row and in mean, other rows unaffected.
 * vals (B); mean (1, may be NULL): the batch mean; corr (B, 2, L) fp64, may be
 * NULL: r then b as the solve sees them.  No atomics: the same bits run to run.
 * sel_bss_sdr_chunk: samples of n per correlation block (host). */
int64_t sel_bss_sdr_chunk(void);
size_t sel_bss_sdr_workspace(int64_t B, int64_t T, int filter_length);
int sel_bss_sdr(const float* pred, const float* target, int64_t B, int64_t T, int filter_length, int zero_mean,
                double load_diag, float* vals /*B*/, float* mean /*1, may be NULL*/,
                double* corr /*(B, 2, filter_length), may be NULL*/, void* ws, size_t ws_bytes,
                sel_stream_t stream);

/* ---- ragged batches: per-row lengths through the measures ----
 * lengths: a DEVICE array of B int64.  T stays the row stride and the largest
 * length; row b is its first lengths[b] samples and nothing at or past
 * lengths[b] influences any output (the padding may hold NaN).  The host never
 * reads lengths, so the contract on its values is kept on the device: a value
 * above T counts as T; a row shorter than the measure's minimum (1 for the SDR
 * family, the BSS-eval SDR and rows_l1_l2; 256 for STOI; n_fft / 2 + 1 for
 * power-mel) is NaN in that row and in the batch mean and leaves the other
 * rows alone.  Each *_var call takes the arguments of its fixed-length form
 * plus lengths, refuses what that form refuses (and null lengths) before any
 * device work, uses the same workspace size, allocates nothing, never reads
 * the device from the host, can be captured, uses no atomics and gives the
 * same bits run to run.  Row b of a ragged call has the bits of the
 * fixed-length call on that row alone at T = lengths[b]; the batch mean is the
 * mean of the per-row values.
 *   sel_sdr_bwd_var writes all of g_pred (B, T), exact zeros at and past lengths[b].
 *   sel_stoi_var: (lengths[b] - 256) / 128 + 1 frames per row; info reports each
 *     row's own (frames, kept, M).  Forward only.
 *   sel_resample_var: row b is resampled as a signal of lengths[b] samples;
 *     y (n_wavs, sel_resample_out_len(len, ...)) is zero at and past
 *     out_lengths[b] = sel_resample_out_len(lengths[b], ...) (device, int64).
 *   sel_power_mel_fwd_var: the reflect pad mirrors about lengths[b] - 1; row b
 *     has frames[b] = 1 + lengths[b] / hop frames (device, int64), the frames of
 *     out (B, n_mels, 1 + T / hop) past them are zero.
 *   sel_rows_l1_l2_var: row b of a and b is `inner` sub-rows of `stride`
 *     elements, of which the first n[b] count: l1[b] = mean |a - b|, l2[b] =
 *     mean (a - b)^2 over inner * n[b] elements, fp64 sums in a fixed order;
 *     means (2, may be NULL): the batch means of l1 and l2. */
int sel_sdr_fwd_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int scale_invariant, int zero_mean, float* vals /*B*/, float* mean /*1*/, void* ws,
                    size_t ws_bytes, sel_stream_t stream);
int sel_sdr_bwd_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int scale_invariant, int zero_mean, const float* g_vals /*B, may be NULL*/,
                    const float* g_mean /*1, may be NULL*/, float* g_pred, const void* ws, size_t ws_bytes,
                    sel_stream_t stream);
int sel_stoi_var(const float* clean, const float* proc, int64_t B, int64_t T, const int64_t* lengths, int extended,
                 float* d /*B*/, float* mean /*1, may be NULL*/, int* info /*3B, may be NULL*/, void* ws,
                 size_t ws_bytes, sel_stream_t stream);
int sel_bss_sdr_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int filter_length, int zero_mean, double load_diag, float* vals /*B*/,
                    float* mean /*1, may be NULL*/, double* corr /*(B, 2, filter_length), may be NULL*/, void* ws,
                    size_t ws_bytes, sel_stream_t stream);
int sel_resample_var(const float* x, int64_t n_wavs, int64_t len, const int64_t* lengths, int orig_freq,
                     int new_freq, int lowpass_filter_width, float rolloff, const float* table, float* y,
                     int64_t* out_lengths /*n_wavs*/, sel_stream_t stream);
int sel_power_mel_fwd_var(const float* x, int64_t B, int64_t T, const int64_t* lengths, int n_fft, int hop,
                          int win_length, const float* window, const float* fb, const int32_t* krange, int n_mels,
                          float power, float* out, int64_t* frames /*B*/, sel_stream_t stream);
int sel_rows_l1_l2_var(const float* a, const float* b, int64_t B, int64_t inner, int64_t stride, const int64_t* n,
                       float* l1 /*B*/, float* l2 /*B*/, float* means /*2, may be NULL*/, sel_stream_t stream);

/* ---- data pipeline: band-limited resampling ----
 * replaces torchaudio.functional.resample(x, orig, new) at dataloader/AudioDataset.py:28-33
 * (defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; torchaudio 2.1.1
 * restated).  x (n_wavs, len) fp32 -> y (n_wavs, sel_resample_out_len(len, ...)).
 * The tap table [phases][taps] is caller-owned: fill it on the host with
 * sel_resample_kernel and copy it to the device. */
int sel_resample_plan(int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, int* phases,
                      int* taps);
int64_t sel_resample_out_len(int64_t len, int orig_freq, int new_freq);
int sel_resample_kernel(int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, float* table);
int sel_resample(const float* x, int64_t n_wavs, int64_t len, int orig_freq, int new_freq, int lowpass_filter_width,
                 float rolloff, const float* table, float* y, sel_stream_t stream);
/* The transpose of sel_resample for the same plan and table: gy (n_wavs,
 * sel_resample_out_len(len, ...)) -> gx (n_wavs, len) = K^T gy.  One thread per
 * input sample gathers its output frames and phases in ascending order (no
 * atomics); every element of gx is written.  Refusals as sel_resample. */
int sel_resample_bwd(const float* gy, int64_t n_wavs, int64_t len, int orig_freq, int new_freq,
                     int lowpass_filter_width, float rolloff, const float* table, float* gx, sel_stream_t stream);

/* ---- waveform shape loss (losses/waveform_loss.py:15-74), one window length per call ----
 * L1(maxpool_w(|y_hat|), maxpool_w(|y|)) over (rows, T) -> out[0]; argidx/dsign
 * (rows * (T / w) each) carry the argmax and sign(diff) to the backward, which
 * ADDS g_out[0] * g_mul * d loss / d y_hat into g_yhat (y is not differentiated). */
size_t sel_shape_loss_workspace(int64_t rows, int64_t T, int win);
int sel_shape_loss_fwd(const float* y_hat, const float* y, int64_t rows, int64_t T, int win, int32_t* argidx,
                       float* dsign, float* out, void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_shape_loss_bwd(const float* y_hat, int64_t rows, int64_t T, int win, const int32_t* argidx,
                       const float* dsign, const float* g_out, float g_mul, float* g_yhat, sel_stream_t stream);

/* ---- HiFi-GAN discriminator (GAN mode) ------------------
 * models/vocoder/HiFiGAN.py:308-395 (Discriminator), models/vocoder/modules/
 * discriminator.py:26-447 (HiFiGANPeriod/Scale discriminators and their multi-
 * versions), losses/adversarial_loss.py:13-124, losses/feat_match_loss.py:13-55.
 *
 * One conv primitive over channels-last rows covers every layer and adjoint:
 *   out[b, j, col(g,o)] = sum_{i<K, r<S, c<Cg} Wp[g][o][i][r][c] * x[b, j+q0+i, r*Cs + g*Cg + c]
 * (input rows outside [0, Tv) read as 0), col(g, o) = (o / Ng)*Ns + g*Ng + o % Ng.
 * Strided convs run on the phase view of their input (S = stride phases of C
 * channels per row, Cs = C), their adjoints with So = stride output phases.
 * Epilogue: + bias[col], then (+ res) * LeakyReLU'(aux) when aux != NULL, then
 * LeakyReLU(slope) when act = 1; rows j in [Tvalid, Tvo) are written as 0. */
typedef struct sel_dconv_desc {
  int32_t B;       /* sequences */
  int32_t Tv;      /* input rows per sequence read (rows >= Tv read as 0) */
  int32_t Tvs;     /* input rows allocated per sequence (>= Tv) */
  int32_t ldx;     /* input row pitch (elements) */
  int32_t Tvo;     /* output rows per sequence (allocated) */
  int32_t Tvalid;  /* computed output rows per sequence */
  int32_t ldo;     /* output row pitch (elements) */
  int32_t K;       /* taps */
  int32_t q0;      /* row offset of tap 0 */
  int32_t S, Cs, Cg; /* reduction: S phases (stride Cs columns) x Cg channels per group */
  int32_t G;       /* groups */
  int32_t So, Ns, Ng; /* outputs: So phases (stride Ns columns) x Ng channels per group */
  int32_t act;     /* 0 none, 1 LeakyReLU */
  float slope;     /* LeakyReLU negative slope (nonlinear_activation_params) */
} sel_dconv_desc;
/* kernel family a sel_dconv_fwd launch of this shape takes (the launcher's own
 * decision, current tune knobs included); writes the kernel's name as rocprofv3
 * lists it (template arguments of the tile) into name[cap] when name != NULL.
 * Returns -1 for an invalid descriptor. */
enum {
  SEL_DPATH_VALU = 0,    /* generic VALU kernel */
  SEL_DPATH_MFMA = 1,    /* matrix-core tile, synchronous stages (grouped layers) */
  SEL_DPATH_SHORT = 2,   /* short reduction (1-channel convs), unstaged */
  SEL_DPATH_PF = 3,      /* matrix-core tile with register prefetch (one group, K <= 8) */
  SEL_DPATH_WS = 4,      /* warp-specialised 256 x 128 kernel, per-sequence tiles */
  SEL_DPATH_WS_FLAT = 5, /* warp-specialised kernel, flat tiles across zero-gapped sequences */
  SEL_DPATH_TINY = 6,    /* narrow outputs (<= 4 columns) */
  SEL_DPATH_GPF = 7,     /* grouped matrix-core tile with register-prefetched stages */
  SEL_DPATH_SHORTX = 8   /* short reduction with the input tile staged in LDS */
};
int sel_dconv_kernel(const sel_dconv_desc* d, int dtype, char* name, size_t cap);
int sel_dconv_fwd(const sel_dconv_desc* d, int dtype, const void* x, const void* wpack, const float* bias,
                  const void* aux, const void* res, void* out, sel_stream_t stream);
/* phase-view tap geometry of a torch conv (kernel Kt, stride, symmetric pad):
 * K = floor((Kt-1-pad)/stride) - q0 + 1 taps from row offset q0 = floor(-pad/stride) */
int sel_dconv_geometry(int Kt, int stride, int pad, int* K, int* q0);
/* torch weight w[N][Cg][Kt] (Conv1d, groups G; or Conv2d (Kt,1)), optionally
 * weight-normed (wg != NULL: w = wg[n] * v / ||v_n||, v = w), into the forward
 * form Wp[g][n][i][r][c] (mode 0) or the adjoint form Wd[g][(r,c)][K-1-i][n] (mode 1). */
int sel_dconv_pack(int mode, const float* w, const float* wg, int N, int Cg, int Kt, int stride, int pad, int G,
                   int dtype, void* out, sel_stream_t stream);
/* Batched sel_dconv_pack: many (layer, mode) packs in one launch per 24 jobs
 * (`jobs` is a HOST array; the same arithmetic per element as sel_dconv_pack).
 * mode 2: the adjoint form as the transpose of a forward form (dtype) at `w`,
 * e.g. one packed by a mode-0 job of the same call (run after all mode 0 / 1 jobs). */
typedef struct sel_dpack_job {
  const float* w;    /* torch weight (or weight_v); mode 2: the packed forward form */
  const float* wg;   /* weight_g or NULL */
  void* out;         /* packed form (dtype) */
  int32_t mode, N, Cg, Kt, stride, pad, G, reserved;
} sel_dpack_job;
int sel_dconv_pack_many(const sel_dpack_job* jobs, int njobs, int dtype, sel_stream_t stream);
/* weight/bias gradient of a forward layer descriptor (So = 1): gw[N][Cg][Kt] fp32
 * in the torch layout, or, with weight norm (v = the weight_v parameter, wg =
 * weight_g): gw = dL/dv and gg[N] = dL/dg; gb[N] = sum of gout when non-NULL. */
size_t sel_dconv_wgrad_workspace(const sel_dconv_desc* d, int dtype);
int sel_dconv_wgrad(const sel_dconv_desc* d, int dtype, const void* gout, const void* x, int N, int Cg, int Kt,
                    int stride, int pad, const float* v, const float* wg, float* gw, float* gg, float* gb, void* ws,
                    size_t ws_bytes, sel_stream_t stream);
/* The weight-gradient kernel a forward layer descriptor (So = 1) takes and how
 * its rows are split (the launcher's own decision, current tune knobs included;
 * no GPU needed): the kernel's name as rocprofv3 lists it into name[cap] when
 * name != NULL, and plan = {nsplit, 128- or 64-row tiles (k_dwgrad_w3 /
 * k_dwgrad_mfma) or rows (the others) per split, bias partials the final
 * reduction reads, row pitch of k_dwgrad_w3's flat tiling (0: per-sequence
 * tiles)} when plan != NULL.  Returns -1 for an invalid descriptor. */
int sel_dconv_wgrad_kernel(const sel_dconv_desc* d, int dtype, char* name, size_t cap, int32_t plan[4]);
/* The (NT, CT, MAXT) instances of k_dwgrad_w3 the library holds, 3 ints each
 * into triples[3 * cap] (NULL: count only); returns their number. */
int sel_dconv_w3_instances(int32_t* triples, int cap);
/* sel_dconv_wgrad in two phases, so that several layers' final reductions run
 * as one launch: _partials writes the split partials into ws (which must stay
 * allocated, in stream order, until the finish) and describes the reduction
 * in *job; _finish_many runs the reductions of njobs layers (gw / gg / gb as
 * sel_dconv_wgrad writes them). */
typedef struct {
  const float* part;   /* folded split partials (in the layer's ws) */
  const float* bpart;  /* bias partials or NULL */
  const float* v;      /* weight_v or NULL */
  const float* wg;     /* weight_g or NULL */
  float* gw;
  float* gg;
  float* gb;
  int32_t N, Cg, Kt, stride, pad, G, nsplit, bsplit;
} sel_dwgrad_job;
int sel_dconv_wgrad_partials(const sel_dconv_desc* d, int dtype, const void* gout, const void* x, int N, int Cg,
                             int Kt, int stride, int pad, const float* v, const float* wg, float* gw, float* gg,
                             float* gb, void* ws, size_t ws_bytes, sel_dwgrad_job* job, sel_stream_t stream);
int sel_dconv_wgrad_finish_many(const sel_dwgrad_job* jobs, int njobs, sel_stream_t stream);
/* AvgPool1d(kernel, stride, padding, count_include_pad) between MSD scales
 * (discriminator.py:428-447): (B, T) rows of pitch ldx -> (B, To) rows of pitch ldo
 * (positions >= To zero-filled); backward overwrites gx. */
int sel_avgpool1d_fwd(const float* x, int B, int T, int ldx, int kernel, int stride, int pad, int To, int ldo,
                      float* y, sel_stream_t stream);
int sel_avgpool1d_bwd(const float* gy, int B, int T, int ldx, int kernel, int stride, int pad, int To, int ldo,
                      float* gx, sel_stream_t stream);
/* MPD front-end (discriminator.py:120-126): reflect-pad T to a multiple of the
 * period, (B, 1, T/p, p) -> B*p sequences of L = ceil(T/p) rows (pitch Lalloc,
 * rows >= L zero); unfold = the adjoint (folds the reflect pad), overwrites gx. */
int sel_mpd_fold(const float* x, int B, int T, int ldx, int period, int Lalloc, float* y, sel_stream_t stream);
int sel_mpd_unfold(const float* gy, int B, int T, int ldx, int period, int Lalloc, float* gx, sel_stream_t stream);
/* GAN loss reductions over strided views (ndim <= 4, sizes/strides in elements,
 * host arrays): kind 0 = sum|a-b| (feat_match_loss.py:46), 1 = sum (a-target)^2
 * (adversarial_loss.py:57/115/118), 2 = sum min(a-1,0), 3 = sum min(-a-1,0)
 * (hinge, :121/:124), 4 = sum a (generator hinge -mean, :60).  out[0] (+)= scale * sum.  grad (+)= gscale[0] * mult *
 * d(term)/da elementwise (gscale: device scalar, the upstream gradient). */
size_t sel_gan_workspace(void);
int sel_gan_reduce(int kind, int dtype, const void* a, const int64_t* a_size, const int64_t* a_stride,
                   const void* b, const int64_t* b_size, const int64_t* b_stride, int ndim, float target,
                   double scale, int accumulate, float* out, void* ws, size_t ws_bytes, sel_stream_t stream);
int sel_gan_grad(int kind, int dtype, const void* a, const int64_t* a_size, const int64_t* a_stride, const void* b,
                 const int64_t* b_size, const int64_t* b_stride, int ndim, float target, const float* gscale,
                 float mult, void* grad, const int64_t* g_stride, int accumulate, sel_stream_t stream);

/* ---- HiFi-GAN vocoder generator, inference (models/vocoder/HiFiGAN.py:28-305,
 * modules/residual_block.py:23-106, modules/multi_fusion.py:23-141) ----------
 * Every conv of the generator is ONE grouped primitive with the channels-last
 * lowering of sel_conv_desc (row(m,k) = b*T + t + k*dil - pad, t = m % T_out,
 * b = m / T_out; SEL_PAD_ZERO / SEL_PAD_REPLICATE; packed weights Wp[N][K][C/G],
 * i.e. per group g the block Wp[g*N/G .. (g+1)*N/G): sel_pack_weight kinds
 * SEL_PACK_FWD (cout = N, cin = C/G) and SEL_PACK_CONVT serve it):
 *   out[m, n] = epi( sum_{k<K} sum_{c<C/G} Wp[n][k][c] * act(in[row(m,k), g*in_group_stride + c]) ),
 *   g = n / (N/G);
 *   act(v) = v >= 0 ? v : act_slope * v  (act_slope 1 = identity); input rows
 *   t < act_skip of each sample are taken as they are (a streaming buffer that
 *   already holds activated rows, conv_layer.py:144-147 fed by HiFiGAN.py:289);
 *   epi(v): v += bias[n % bias_period]; v += res[m, g*res_group_stride + n % (N/G)]
 *   when res != NULL; v = tanh(v) when tanh_out; v *= out_scale; v += out[m, n]
 *   (the value already there) when accumulate.
 * in_group_stride is C/G (input rows of pitch C), or 0: every group reads the
 * same C/G channels of an input of pitch C/G -- MultiGroupConv1d's
 * x.repeat(1, groups, 1) (multi_fusion.py:124) without the copy; res_group_stride
 * likewise (N/G with pitch N, or 0 with pitch N/G).  T input rows and T_out
 * output rows per sample (T_out 0: = T); T_out < T with pad 0 is the valid
 * conv of a streaming step.  Rows outside [0, T) of the sample read 0, or the
 * sample's first / last row in replicate mode: never another sample's rows.
 * CONTRACT (bf16): the prologue result act(v) is rounded to bf16 once before
 * the matrix multiply; products accumulate in fp32; res, the accumulated
 * out and the result are rounded to the output type once each.
 * in_dtype / out_dtype: fp32 -> fp32, bf16 -> bf16 or fp32; res and an
 * accumulated out have the output type. */
typedef struct sel_hfg_conv_desc {
  int64_t rows;             /* B * T_out */
  int32_t T;                /* input rows per sample */
  int32_t T_out;            /* output rows per sample, 0: T */
  int32_t C, N;             /* in / out channels over all groups */
  int32_t K, dil, pad;
  int32_t pad_mode;         /* SEL_PAD_* */
  int32_t groups;
  int32_t in_group_stride;  /* C/G or 0 */
  int32_t res_group_stride; /* N/G or 0 */
  int32_t bias_period;      /* 0: no bias */
  int32_t act_skip;
  int32_t tanh_out;
  int32_t accumulate;
  float act_slope;
  float out_scale;
} sel_hfg_conv_desc;
/* kernel a launch of this shape takes: 0 = one thread per output (fp32, thin
 * outputs with N/G <= 4, tiles that do not fit LDS), 1 / 2 / 4 = the bf16
 * matrix-core tile of 64 rows x 16 / 32 / 64 channels; negative: bad descriptor */
int sel_hfg_conv_kernel(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype);
int sel_hfg_conv_fwd(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* in, const void* wpack,
                     const float* bias, const void* res, void* out, sel_stream_t stream);
/* Fused residual layer (residual_block.py:93-97, one launch per layer):
 *   out = epi( x + conv2_{K,1}(act(conv1_{K,dil}(act(x)) + b1)) + b2 ),
 * d1 describes conv1 (causal zero pad (K-1)*dil, C = N, groups, in_group_stride,
 * act_slope) and the final epilogue (x is the residual: res_group_stride 0
 * exactly when in_group_stride is 0; out_scale, accumulate); conv2 has the same
 * K and groups at dilation 1; b1 and b2 both given or bias_period 0.  The conv1
 * tile with the K-1 halo rows conv2 needs stays in LDS.  bf16, C/G in {32, 64},
 * K in {3, 7, 11}, any dil whose tiles fit LDS; bit-identical to the two
 * sel_hfg_conv_fwd launches it replaces (same MFMA sequence, h rounded to bf16
 * where the first launch would store it).  Returns SEL_ERR_UNSUPPORTED for every
 * other shape and for the (C/G, K) pairs on which two launches measured no
 * slower -- the caller then issues the two launches.  sel_tune key 71: 1 =
 * always SEL_ERR_UNSUPPORTED (the two-launch path), 2 = fused wherever the
 * shape allows (A/B runs, tests). */
int sel_hfg_reslayer_fwd(const sel_hfg_conv_desc* d1, int dtype, const void* x, const void* w1pack, const float* b1,
                         const void* w2pack, const float* b2, void* out, sel_stream_t stream);

/* ---- HiFi-GAN vocoder generator, streaming step (HiFiGAN.py:266-305
 * StreamGenerator.decode, residual_block.py:100-106, multi_fusion.py:119-141) --
 * One causal layer of one vocoder hop on channels-last rows: the grouped
 * primitive of sel_hfg_conv_fwd with the reference's pad_buffer as an explicit
 * carry, as sel_conv_step is to sel_conv_fwd.  Same descriptor:
 *   T = d->T NEW rows per sample, B = d->rows / T, P = (K-1)*dil;
 *   required (SEL_ERR_ARG otherwise): T_out 0 or T, pad == P, pad_mode
 *   SEL_PAD_ZERO, act_skip == 0 (the carry is the skipped part);
 *   v[b] = [ carry[b] (P rows of pitch C) | act(in[b]) (T rows) ],
 *          act(x) = x >= 0 ? x : act_slope * x on the NEW rows only: the carry
 *          holds what pad_buffer holds, the ACTIVATED tail (act_slope 1 = identity);
 *   out[m, n] = epi( sum_{k<K} sum_{c<C/G} Wp[n][k][c] * v[b, t + k*dil, g*(C/G) + c] ),
 *          g = n / (N/G), m = b*T + t, epi as sel_hfg_conv_fwd and in its order:
 *          + bias[n % bias_period], + res[m, g*res_group_stride + n % (N/G)],
 *          tanh when tanh_out, * out_scale, + out[m, n] when accumulate;
 *   in_group_stride 0: the new rows have pitch C/G and every group reads them
 *          (MultiGroupConv1d's x.repeat(1, groups, 1) without the copy).  The
 *          carry ALWAYS has pitch C (it stands for a state_dict entry), so
 *          carry_out then holds the activated new rows once per group.
 *          res_group_stride 0 likewise: res of pitch N/G;
 *   carry_out[b] = the last P rows of v[b], in in_dtype, written with the act()
 *          the operand uses: bit for bit what the conv consumed (T < P keeps
 *          P - T rows of the old carry).  carry is never written; carry_out must
 *          not alias carry, in or res, out must not alias any input (SEL_ERR_ARG).
 *          K = 1: P = 0, carry and carry_out may be NULL.
 * Wp is what sel_pack_weight writes: SEL_PACK_FWD with cin = C/G for the causal
 * convs; SEL_PACK_CONVT for the upsampling layers, a 2-tap conv with N = s*Cout,
 * P = 1 and bias_period = Cout, out viewed as (T*s, Cout).
 * CONTRACT (bf16), as sel_hfg_conv_fwd: act(v) is rounded to bf16 once, products
 * accumulate in fp32; res, the accumulated out and the result are rounded to
 * the output type once each.  in_dtype / out_dtype: fp32 -> fp32, bf16 -> bf16
 * or fp32; res and an accumulated out have the output type.
 * Any C/G and N/G: ceil((N/G)/16) masked column tiles per group; (C/G) % 8 == 0
 * with 16-byte aligned pointers takes 16-byte operand loads.  The K*(C/G)
 * reduction is split over the waves of a block by K*(C/G) alone and summed in
 * wave order: no atomics, no workspace, two calls give the same bits, and an
 * output does not depend on B, T or the group count.  Arguments (C % G, N % G,
 * the group strides, the dtypes, the aliasing rules) are validated before any
 * device work. */
int sel_hfg_conv_step(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* carry, const void* in,
                      const void* wpack, const float* bias, const void* res, void* out, void* carry_out,
                      sel_stream_t stream);
/* sel_hfg_conv_step with a slot table, exactly as sel_conv_step_pool extends
 * sel_conv_step: d->rows = capacity * T, dense in / res / out in active order
 * (in_group_stride / res_group_stride 0, accumulate, tanh_out and out_scale as
 * in the session form; an accumulated out is read and written for the first
 * n*T rows only), carry / carry_out pools of nslots slot rows of pitch P*C
 * (the carry pitch is C, as now), n = min(*n_active, capacity), early return of
 * row groups at or beyond n*T, entries outside [0, nslots) absent.  Bit for
 * bit sel_hfg_conv_step at B = 1 per sample. */
int sel_hfg_conv_step_pool(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* carry,
                           void* carry_out, int nslots, const int32_t* slots, const int32_t* n_active,
                           const void* in, const void* wpack, const float* bias, const void* res, void* out,
                           sel_stream_t stream);

/* ---- HiFi-GAN vocoder generator, backward of the grouped primitive ---------
 * Same descriptor, same channels-last lowering.  Write the forward as
 *   out = prev*[accumulate] + out_scale * tanh?( conv(act(x)) + bias + res );
 * gpre = out_scale * gout * (1 - out^2 when tanh_out) is the gradient at the
 * conv's own output (before bias and res).  Training never streams: T_out not in
 * {0, T} or act_skip != 0 returns SEL_ERR_UNSUPPORTED.  Descriptors are validated
 * before any device work.  in_dtype is the type of x, the weights and gin;
 * out_dtype that of gout and the saved out (fp32 for the tanh output conv).
 *
 * sel_hfg_conv_bwd_data: the exact adjoint of the forward gather, then the
 * activation derivative, then the skip:
 *   gin[b, s, g*igs + c] = act'(x[b,s,.]) * sum_{(t,k): in_row(t + k*dil - pad) = s} sum_{n in group g}
 *                          W[n][k][c] * gpre[b,t,n]  +  skip_scale * gskip-term  +  gin_prev*[accumulate].
 *   Pad adjoints: under SEL_PAD_ZERO taps outside [0, T) contribute nothing; under
 *   SEL_PAD_REPLICATE the clamped taps add to the edge rows (the 2-tap transposed
 *   form: row 0 also receives W[k=0]^T gpre[0]).  A gradient never crosses a
 *   sample boundary.  act'(v) = 1 for v > 0, else act_slope (so act_slope at
 *   v == 0, torch's convention); x may be NULL when act_slope is 1.
 *   in_group_stride 0 (shared input): gin has C/G channels and is the sum over all
 *   groups -- the adjoint of MultiGroupConv1d's repeat without a G-wide temporary.
 *   gskip (may be NULL): the gradient arriving through a residual connection
 *   that read the same x; it has pitch C and is added after the mask, times
 *   skip_scale: gskip[m, g*C/G + c] with in_group_stride C/G, the sum over g of
 *   those entries with in_group_stride 0.  The desc's accumulate adds the result to
 *   the gin already there (the MultiReceptiveField blocks all feed one gx); its
 *   res_group_stride and bias_period are not used.  `out` is read only with tanh_out.
 *   Weights: wdpack = Wp with the outer and inner axis of each group block
 *   exchanged, Wd[G][C/G][K][N/G] (same values, no rounding), so that the
 *   reduction axis is contiguous.
 *   bf16 contract: gout and W are bf16 operands as stored, products accumulate in
 *   fp32, out_scale, mask, skip and accumulate are applied in fp32, gin is
 *   rounded once.
 *
 * sel_hfg_conv_wgrad: gwpack[n][k][c] = sum_{b,t} gpre[b,t,n] * act(x[b, in_row(t + k*dil - pad), g*igs + c])
 * in the packed layout Wp[N][K][C/G], always fp32 (sel_unpack_wgrad with
 * SEL_PACK_FWD, cout = N, cin = C/G, or SEL_PACK_CONVT returns it to the torch
 * layout); act(x) is rounded to bf16 once in the bf16 instance, as the forward
 * does.  gbias (given exactly when bias_period > 0) [j] = sum of gpre[., n] over all n = j (mod
 * bias_period): the transposed form sums its s output phases.  The rows are
 * split over 64-row tiles into fixed-order partials in ws
 * (sel_hfg_conv_wgrad_workspace bytes) with a fixed-order finish: no float
 * atomics, two runs are bit-identical.  sel_tune key 72 > 0 forces the split
 * count (clamped to the number of row tiles).
 *
 * sel_hfg_conv_bwd_kernel: the instance a shape takes.  wgrad 0, the data
 * gradient: 0 = one thread per gin element (fp32, the tanh conv, C/G or N/G <= 4,
 * tiles that do not fit LDS), 1 / 2 / 4 = the bf16 matrix-core tile of 64 rows x
 * 16 / 32 / 64 channels.  wgrad 1: 0 = one thread per weight element and split,
 * 1 = the bf16 matrix-core kernel.  Negative: bad descriptor. */
int sel_hfg_conv_bwd_kernel(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, int wgrad);
int sel_hfg_conv_bwd_data(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* gout, const void* out,
                          const void* x, const void* wdpack, const void* gskip, float skip_scale, void* gin,
                          sel_stream_t stream);
size_t sel_hfg_conv_wgrad_workspace(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype);
int sel_hfg_conv_wgrad(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* gout, const void* out,
                       const void* x, float* gwpack, float* gbias, void* ws, size_t ws_bytes, sel_stream_t stream);

/* ---- UnivNet spectral discriminator: channels-last 2-D conv ---------------
 * models/vocoder/modules/discriminator.py:450-580 (UnivNetSpectralDiscriminator):
 * Conv2d(Cin, Cout, (kh, kw), stride (sh, sw)), valid padding, over
 * x (B, H, W, Cin) rows (H frames, W frequency bins) ->
 * y (B, H - kh + 1, (W - kw) / sw + 1, Cout), then LeakyReLU(slope) when act.
 *
 * Limits (anything else returns SEL_ERR_ARG naming the limit, before any device
 * work): kh <= 3, kw <= 9, sh = 1, sw in {1, 2}, kw >= sw; channels 1 -> C,
 * C -> C' or C -> 1 with C, C' multiples of 32, at most 256.
 *
 * Element types: `dtype` (SEL_F32 / SEL_BF16) is the type of every activation
 * with C > 1 channels; the 1-channel tensors (the magnitudes entering a 1 -> C
 * layer and their gradient, the output of a C -> 1 layer and its gradient) are
 * always fp32.  Products accumulate in fp32.
 *
 * Packed weights (written by the caller from the effective weight
 * w (Cout, Cin, kh, kw), sel/sconvops.py):
 *   forward  C -> C':  fp32: wpack[kh][kw][Cout][Cin]; bf16: wpack[2][kh][kw][Cout][Cin],
 *            the bf16 rounding of w and then the bf16 rounding of its remainder
 *            w - bf16(w) (two bf16 matrix products per tap, so the pre-activations
 *            -- and with them the LeakyReLU masks the backward reuses -- carry the
 *            rounding of the stored activations only);
 *            1 -> C and C -> 1:  wpack[kh][kw][C] fp32.
 *   adjoint: for each input-column phase p < sw, the taps kw = p (mod sw)
 *            flipped on both axes, Kp = ceil((kw - p) / sw) of them per row,
 *            phases concatenated:  C -> C': [kh][Kp][Cin][Cout] in `dtype`;
 *            1 -> C and C -> 1: [kh][Kp][C] fp32.
 *
 * sel_sconv_bwd_data: gx = adjoint(gy) (a gather per phase, no atomics), times
 * LeakyReLU'(aux) when aux (the stored output of the previous layer, i.e. this
 * layer's input, same layout as gx) is given.  Input columns no tap reads get
 * an exact 0.
 * sel_sconv_wgrad: gw (Cout, Cin, kh, kw) and gb (Cout; may be NULL), fp32, of
 * the effective weight: per-block partials over contiguous ranges of output
 * rows in ws (sel_sconv_wgrad_workspace bytes), then a fixed-order sum: no
 * atomics, two runs give identical bits. */
typedef struct sel_sconv_desc {
  int32_t B, H, W;      /* input rows (frames) and columns (bins) */
  int32_t Cin, Cout;
  int32_t kh, kw, sh, sw;
  int32_t act;          /* forward: LeakyReLU(slope) after the bias */
  float slope;
} sel_sconv_desc;
int sel_sconv_check(const sel_sconv_desc* d); /* the limits above; no device work */
int sel_sconv_fwd(const sel_sconv_desc* d, int dtype, const void* x, const void* wpack, const float* bias, void* y,
                  sel_stream_t stream);
int sel_sconv_bwd_data(const sel_sconv_desc* d, int dtype, const void* gy, const void* wadj, const void* aux,
                       void* gx, sel_stream_t stream);
size_t sel_sconv_wgrad_workspace(const sel_sconv_desc* d, int dtype);
int sel_sconv_wgrad(const sel_sconv_desc* d, int dtype, const void* gy, const void* x, float* gw, float* gb, void* ws,
                    size_t ws_bytes, sel_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEL_H_ */
