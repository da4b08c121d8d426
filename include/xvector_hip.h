/*
 * xvector_hip.h - C-ABI of the MI355X (gfx950) x-vector training/extraction hot path.
 *
 * The reference (mycrazycracy/tf-kaldi-speaker) has NO native/FFI interface on this
 * path: its hot path is a TF1 graph built by model/tdnn.py:33-191, model/pooling.py:9-34,
 * model/loss.py:9-355 and run by model/trainer.py:505-508 (sess.run(train_op)).  This
 * header is therefore the boundary that the drop-in Python `Trainer`
 * (tf_kaldi_speaker_amd/model/trainer.py) binds through ctypes; every entry point names
 * the reference call site(s) whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  All data pointers are DEVICE
 *     pointers (HBM) unless the name starts with h_.  All tensors are fp32 row-major,
 *     labels int32.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call
 *     only ENQUEUES work; nothing synchronises unless stated.
 *   - return 0 on success, non-zero on error; xv_last_error() gives the message of the
 *     last failing call on the calling thread.
 *   - an engine handle is single-threaded (one TF session per Trainer, trainer.py:24).
 *
 * "Spliced view": a frame-level activation tensor x[B][T][C] is consumed by a layer with
 * context width k as the matrix whose row (b,t) is the contiguous span x[b][t..t+k-1][:]
 * (k*C floats) - rows overlap in memory, nothing is materialised (no im2col).  k = 1 is a
 * plain dense layer.
 */
#ifndef XVECTOR_HIP_H
#define XVECTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: xv_config starts with struct_bytes (round 5).  3: xv_engine_arena_bytes (round 6).  Bumped whenever xv_config's layout or an entry point's signature changes: a host
 * built against another header must fail at load (xv_abi_version) or at xv_engine_create (struct_bytes), never read fields past the end
 * of a shorter struct.  xv_frontend came later and left it at 3: a new entry point beside the old ones, xv_config untouched - a host
 * built against the earlier header runs unchanged against this library.  The same holds for xv_mfcc_num_frames, xv_mfcc_table_floats,
 * xv_mfcc_tables, xv_mfcc and xv_energy_vad, which bring their own struct (xv_mfcc_config, size-checked like xv_config), and for
 * xv_debug_augment_plan, xv_augment_workspace_bytes and xv_augment with theirs (xv_augment_config), and for xv_resample_num_samples,
 * xv_resample_table_floats, xv_resample_tables, xv_debug_resample_plan and xv_resample with theirs (xv_resample_config), and for xv_fbank_num_frames,
 * xv_fbank_table_floats, xv_fbank_tables and xv_fbank with theirs (xv_fbank_config). */
#define XV_ABI_VERSION 3

const char* xv_last_error(void);
int xv_abi_version(void);
/* number of visible HIP devices (0 when none / driver missing); never throws */
int xv_device_count(void);

/* Live kernel timing for bench.py's roofline leg: while enabled, every launch of the three MFMA
 * GEMM kernels is bracketed by hipEvents on the stream it is launched on.
 *   kind 0 = xv_gemm_nt_kernel<true, *> / xv_gemm_nt_sk_kernel<true, *>   (forward conv/dense + BN-statistics epilogue)
 *   kind 1 = xv_gemm_nt_kernel<false, *> / xv_gemm_nt_sk_kernel<false, *> (data gradients, logits)
 *   kind 2 = xv_gemm_tn_kernel        (weight gradients)
 *   kind 3 = xv_gemm16_nt_kernel<true>, kind 4 = xv_gemm16_nt_kernel<false>, kind 5 = xv_gemm16_tn_kernel
 *            (the same three roles on fp16 hi/lo planes, XV_PRECISION_F16X3)
 * xv_profile_end synchronises the recorded events and returns, per kind, the number of launches,
 * their summed duration in ms and their summed algorithmic FLOPs (2*M*N*K each). */
int xv_profile_begin(int max_launches);
/* Same, restricted to the kinds whose bit is set in kind_mask (bit k = kind k): an event pair costs a few
 * microseconds of queue time per launch, so bench.py's timed region brackets only the dominant kernel. */
int xv_profile_begin_kinds(int max_launches, uint32_t kind_mask);
#define XV_PROFILE_KINDS 6
int xv_profile_end(int64_t launches[XV_PROFILE_KINDS], double ms[XV_PROFILE_KINDS], double flops[XV_PROFILE_KINDS]);
/* Diagnostics: the schedule xv_affine_forward / xv_affine_dgrad pick for C[M][N] = A[M][K] . Bt[N][K]^T given ample workspace
 * (stats: the launch emits BatchNorm statistics = a forward launch; co_running: a data gradient beside the weight-gradient stream):
 * 0 one workgroup per tile (xv_gemm_nt_kernel), 1 the evenly scheduled kernel (xv_gemm_nt_sk_kernel), 2 whole tiles + shares of the
 * remaining tiles (xv_gemm_nt_kernel), 3 split-K + slab sum.  tools/pmc_traffic.py attributes layers to kernels with it. */
int xv_debug_nt_schedule(int M, int N, int K, int stats, int co_running);
/* Diagnostics: the plan xv_affine_wgrad (direct = 0) and the engine's loss-head weight gradient (direct = 1: an unsplit result is stored
 * straight into the destination) run for P[M][N] = sum_r A[r][M] . B[r][N] over R reduction rows.  out[0]: 0 the general kernel
 * (xv_gemm_tn_kernel), 1 the 129 ... 160-row kernel (xv_gemm_tn160_kernel); out[1]: splits (slabs summed by the reduce launch);
 * out[2]: reduction rows per split (a multiple of 16); out[3]: 1 when the general kernel stages two K-steps ahead.  Host arithmetic. */
int xv_debug_tn_plan(int M, int N, int R, int direct, int out[4]);
/* Diagnostics: the form of the margin / cross-entropy row kernel xv_margin_softmax_rows (and the engine's loss) runs for a logits pitch of
 * ldl floats with logits and dlogits at those addresses: 8 or 16 (the row held in registers, RQ float4 per thread: ldl % 4 == 0, both
 * addresses 16-byte aligned, ldl <= 8192 or 16384), 0 (three passes over memory: any other pitch or alignment).  Host arithmetic. */
int xv_debug_softmax_rows_form(int ldl, uintptr_t logits, uintptr_t dlogits);
/* Diagnostics: the form xv_col_stats runs for n columns at a pitch of ldz floats with z and bn_part at those addresses: 4 (rows of whole
 * float4s, one pass over memory: n % 4 == 0, ldz % 4 == 0, both addresses 16-byte aligned) or 1 (the scalar form).  Host arithmetic. */
int xv_debug_col_stats_form(int n, int ldz, uintptr_t z, uintptr_t bn_part);
/* Diagnostics: the launch plan of the BatchNorm (+ activation) backward of rows = segs * t frame rows.  pooled: the upstream gradient is the
 * pooling backward over chunks of pool_t frames (rows % pool_t == 0); pad: zero frames around each segment of dz; relu: the entry point's
 * flag; has_slope / has_dalpha: what xv_set_activation holds; has_wpos / has_weights / has_pamax: which optional pooled inputs are given;
 * split: dz as fp16 planes with a |dz| bound; ext_chunks > 0: reduction partials left by a GEMM epilogue (plain ReLU only).
 * out[0] the reduction form: 0 closed form from the pooled statistics, 1 the pooled pass over z, 2 the plain pass, 3 external partials;
 * out[1] the pooled pass's instantiation (4 activation | 2 slope | 1 frame weights; 0 for the other forms); out[2] statistics per chunk
 * (4 with a slope and a d alpha buffer, else 3); out[3] partial rows (chunks of 64 rows, per pooled chunk in the pooled forms; ext_chunks);
 * out[4] the apply pass: 0 dense (pad == 0 and, pooled, pool_t >= 32), 1 strip, 2 split planes.  Host arithmetic, nothing is launched. */
int xv_debug_bn_bwd_plan(int rows, int pooled, int pool_t, int pad, int relu, int has_slope, int has_dalpha, int has_wpos, int has_weights,
                         int split, int has_pamax, int ext_chunks, int out[5]);
/* Diagnostics: the launch plan of the segment-level GEMM kernel (xv_segment_gemm, xv_segment_affine_bn_forward,
 * xv_segment_dgrad_bn_backward) for an m x n result over k with a workspace of ws_bytes.  out[0] column tiles of 32 (gridDim.x); out[1]
 * splits of k (gridDim.y): 256 / tiles, at most k / 64, no more than ws_bytes holds [128][32] float slabs for, then what the chunk leaves;
 * out[2] k per split, a multiple of 32.  Fails with the launcher's message for a shape the launcher refuses.  Host arithmetic. */
int xv_debug_segment_plan(int m, int n, int k, size_t ws_bytes, int out[3]);
/* Diagnostics: the form xv_att_score runs for rows of n columns at a pitch of ldz floats with zk and query at those addresses: 1 (column
 * quads: n % 4 == 0, ldz % 4 == 0, both addresses 16-byte aligned) or 0 (the scalar form).  Host arithmetic. */
int xv_debug_att_score_form(int n, int ldz, uintptr_t zk, uintptr_t query);
/* Diagnostics: the form xv_affine_forward_f16x3 / xv_affine_dgrad_f16x3 / xv_affine_dgrad_bnstats_f16x3 run for C[M][N] = A . Bt^T over K
 * halfs with A rows of lda halfs in segments of a_rps rows at a pitch of a_pitch rows (the weight planes at a pitch of K).  stats: the launch
 * emits BatchNorm statistics; bwd: it emits the BatchNorm-backward partials; conv_wr: the value of XV_CONV_WR (0 unset, 2 or 4), passed in so
 * that the answer does not depend on the process environment.  out[0] the kernel: 0 generic (xv_gemm16_nt_kernel), 1 context-window
 * (xv_gemm16_nt_conv_kernel: lda % 32 == 0, K = taps * lda, taps >= 2, no bwd, and the x rows of any tile fit its A image:
 * (bm - 1) + (a_pitch - a_rps) * ((bm - 1) / a_rps + 1) + (taps - 1) < bm + 32); out[1] rows of a tile (128 | 256); out[2] taps and out[3]
 * 32-channel chunks (0, 0: generic); out[4], out[5] row and column tiles; out[6] K-steps of 32 halfs; out[7] halfs of the last K-step inside
 * K rounded up to 8.  Fails with the launcher's message for a shape the launcher refuses.  Host arithmetic, nothing is launched. */
int xv_debug_gemm16_nt_form(int M, int N, int K, int lda, int a_rps, int a_pitch, int stats, int bwd, int conv_wr, int out[8]);
/* Diagnostics: the plan xv_affine_wgrad_f16x3 runs for P[M][N] = sum_r A[r][M] . B[r][N] over R reduction rows in segments of rps rows at
 * pitches of a_pitch / b_pitch rows.  out[0] tiles of 128 x 128; out[1] splits (slabs summed by the reduce launch): 512 / tiles, at most
 * half the 32-row stages, at least one, then what the chunk leaves; out[2] reduction rows per split, a multiple of 32; out[3] 1 when the rows
 * are gap-free (both pitches == rps) and the kernel sees one segment of R rows; out[4] 1 when whole stages advance lane offsets (the rps
 * the kernel sees >= 32), 0 when every stage takes the per-row form.  Host arithmetic, nothing is launched. */
int xv_debug_gemm16_tn_plan(int M, int N, int R, int rps, int a_pitch, int b_pitch, int out[5]);

/* dst[r][0..cols) = src[r][0..cols) for r < rows (device to device, pitches in floats). */
int xv_copy_2d(void* stream, float* dst, size_t ldd, const float* src, size_t lds, int rows, int cols);

/* ---------------------------------------------------------------------------------
 * Op level (each is one or two kernel launches; used by the parity tests and the engine)
 * --------------------------------------------------------------------------------- */

/* Bytes of scratch an op-level call may need (upper bound for any op below at these sizes). */
size_t xv_op_workspace_bytes(int rows, int cols_in, int cols_out);

/* Zero-pad the channel axis: dst[r][0..c_dst) = src[r][0..c_src), 0 beyond.  Used to bring
 * the 30-dim MFCC rows (dataset feed of trainer.py:491) to a 16-byte-aligned pitch. */
int xv_pad_channels(void* stream, const float* src, int rows, int c_src, float* dst, int c_dst);

/* Kaldi 'CM ' compressed-matrix decode (dataset/kaldi_io.py:768-812 the codec, :814-867 the row sub-range) of a batch the native loader
 * delivers undecoded (include/xvector_io.h, xvio_config.packed): b chunks of chunk_stride bytes, each
 *   [min f32][range f32][d x (p0, p25, p75, p100) u16][d x t u8, column after column]
 * -> out [b][t][d] float32, bit-identical to the host decoder and the reference reader.  d <= 128. */
int xv_cm_decode(void* stream, const uint8_t* packed, int b, int t, int d, size_t chunk_stride, float* out);
/* Ragged form for whole utterances of different lengths (batched extraction, extract.py:64-93 / kaldi_io.py:768-812 read_mat_ark): chunk i
 * is a 'CM ' matrix of rows[i] <= t frames exactly as it sits in the archive behind the "CM " token - [min f32][range f32][rows i32]
 * [cols i32][d x (p0, p25, p75, p100) u16][d x rows[i] u8, column after column] - at byte offsets[i] of `packed`; it is decoded into
 * out[i][0 .. rows[i]) of the [b][t][d] tensor and the padding rows behind it are zeroed.  offsets / rows: device arrays [b]. */
int xv_cm_decode_ragged(void* stream, const uint8_t* packed, const int64_t* offsets, const int32_t* rows, int b, int t, int d, float* out);

/* Kaldi 'CM ' compressed-matrix ENCODE: what copy-feats --compress=true does at the end of the reference's feature preparation
 * (egs/voxceleb/v1/run.sh stage 4, prepare_feats_for_egs.sh; matrix/compressed-matrix.cc ComputeGlobalHeader / ComputeColHeader /
 * FloatToChar).  THE SPECIFICATION IS dataset/kaldi_io.py write_compressed_mat, BYTE FOR BYTE, in both of its header forms.
 * x: [b][t][d] float32 as xv_mfcc and xv_frontend leave it, piece i holding rows[i] frames, 1 <= rows[i] <= t, d <= 128; rows behind
 * rows[i] are padding and enter no statistic.  Piece i's image - what a 'CM ' matrix is in an archive behind the "CM " token,
 *   [min f32][range f32][rows i32][cols i32][d x (p0, p25, p75, p100) u16][d x rows[i] u8, column after column]
 * (16 + 8 d + d rows[i] bytes), exactly what xv_cm_decode_ragged reads - is written at byte out_offsets[i] of `out`, at ANY alignment
 * (images packed back to back are unaligned as soon as d rows[i] is odd).  rows, out_offsets: device arrays [b]; neither is checked
 * on the device, the caller checks them (ops.cm_encode does).  Every fp32 step below is one operation, rounded once, in the order
 * written, with no contraction; divisions are correctly rounded.
 *   Global header: min and max of the valid elements, exact.  range = fp32(double(max) - double(min)), or, if they are equal,
 *     fp32(double(min) + 1 + |min| - double(min)).
 *   header = XV_CM_HEADER_QUARTILES (Kaldi's choice): per column the order statistics s[k] of its rows[i] values, found exactly.
 *     rows >= 5: s[0], s[rows / 4], s[3 rows / 4], s[rows - 1] (integer division), each mapped by
 *       u16(v) = clamp(floor(((v - min) / range) * 65535 + 0.499), 0, 65535), all fp32, 0.499 rounded to fp32.
 *     rows < 5 (the small-matrix branch): p0 = u16(s[0]); p25 = u16(s[1]) if rows > 1, else p0 + 1; p75 = u16(s[2]) if rows > 2, else
 *       p25 + 1; p100 = u16(s[3]) if rows > 3, else p75 + 1 - the + 1 in uint16 arithmetic: 65535 + 1 = 0, as the host writer's wraps.
 *   header = XV_CM_HEADER_UNIFORM (evenly spaced points; what make_mfcc.py writes): from the column's minimum a and maximum z alone, IN
 *     DOUBLE: p0 = clamp(floor((a - min) / range * 65535)), p100 = clamp(ceil((z - min) / range * 65535)), p25 = rint(p0 + 0.25 (p100 -
 *     p0)), p75 = rint(p0 + 0.75 (p100 - p0)), rint rounding halves to even.
 *   Both: the strictly-increasing fix-up p0 = min(p0, 65532), p25 = min(max(p25, p0 + 1), 65533), p75 = min(max(p75, p25 + 1), 65534),
 *     p100 = max(p100, p75 + 1); the four float points f = min + ((range * fp32(1 / 65535)) * p); per element v: if v < f25 the code is
 *     clamp(floor(((v - f0) / (f25 - f0)) * 64 + 0.5), 0, 64), else if v < f75 64 + floor(((v - f25) / (f75 - f25)) * 128 + 0.5) clamped
 *     to 64 .. 192, else 192 + floor(((v - f75) / (f100 - f75)) * 63 + 0.5) clamped to 192 .. 255.
 * OUTSIDE THE BYTE CONTRACT: (1) where two of a column's four float points coincide in fp32 (its header steps fall below the fp32
 * spacing at the values' magnitude) the host writer divides by zero and casts NaN to uint8, which is platform-defined: for such a column
 * only the header bytes are specified, every code lies inside the range of the branch chosen, nothing faults; (2) inputs are finite;
 * (3) a matrix whose minimum is a zero that occurs with both signs (either zero may come back as the minimum).
 * One launch, one workgroup per piece; integer LDS atomics only, no floating-point atomics, no cross-workgroup hand-over: the bytes
 * depend on the shape of the call only. */
#define XV_CM_HEADER_QUARTILES 0
#define XV_CM_HEADER_UNIFORM 1
int xv_cm_encode(void* stream, const float* x, const int32_t* rows, int b, int t, int d, int header, const int64_t* out_offsets,
                 uint8_t* out);

/* The feature front end of extraction on a decoded batch: sliding-window cepstral mean normalisation, then voiced-frame selection - the
 * two Kaldi programs the reference recipe pipes in front of extract.py (egs/voxceleb/v1/nnet/run_extract_embeddings.sh:47):
 *   apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=W   (featbin/apply-cmvn-sliding.cc, SlidingWindowCmn in
 *                                                                        feat/feature-functions.cc)
 *   select-voiced-frames                                                (ivectorbin/select-voiced-frames.cc)
 * x: [b][t_in][d], piece i holding rows_in[i] raw frames (n below), as xv_cm_decode_ragged leaves them.  out: [b][t_out][d].
 *   CMN (cmn_window = W > 0; 0 = off): for raw frame t, s = t - W/2 (integer division), e = s + W; if s < 0: e -= s, s = 0;
 *     if e > n: s -= e - n, e = n, s = max(s, 0); y[t] = x[t] - mean(x[s:e]), the mean accumulated in double and the difference rounded
 *     to fp32 once.  The window spans RAW frames: voicing does not enter it (in the pipe CMN runs first).
 *   Selection: masks = one byte per raw frame, non-zero = voiced, the masks of all pieces back to back in one buffer of mask_bytes
 *     bytes, piece i's at byte mask_offsets[i] (any alignment; pieces may share a mask); masks = NULL keeps every frame.  With sel the
 *     ascending raw indices of piece i's voiced frames: out[i][j] = y[sel[first[i] + j]] for j < rows_out[i] = min(count[i], |sel| -
 *     first[i]), rows rows_out[i] .. t_out are zero.  first / count (NULL: 0 / t_out) cut a chunk out of the SELECTED frames - how
 *     extract.py:69-79 splits an utterance longer than --chunk-size; every chunk is a piece that holds the whole raw utterance.
 * rows_in, mask_offsets, first, count, rows_out: device arrays [b].  ws: b * t_out * 4 bytes when masks are given (the selected indices;
 * none otherwise) - fewer is an error.  x and out must not overlap.  d <= 128.  Two launches (one without masks), no atomics: the same
 * bits on every call. */
int xv_frontend(void* stream, const float* x, const int32_t* rows_in, int b, int t_in, int d, int cmn_window, const uint8_t* masks,
                size_t mask_bytes, const int64_t* mask_offsets, const int32_t* first, const int32_t* count, int t_out, float* out,
                int32_t* rows_out, void* ws, size_t ws_bytes);

/* MFCC features and the energy VAD from waveforms: the first stage of the recipe, for which the reference goes to Kaldi
 * (egs/voxceleb/v1/run.sh:59-63, egs/sre/v1/run.sh:103-115: steps/make_mfcc.sh --mfcc-config conf/mfcc.conf = compute-mfcc-feats,
 * sid/compute_vad_decision.sh = compute-vad-decision).  Kaldi is not available where this project is built and tested: parity is BY
 * RESTATEMENT - the rules below are the specification, tests/mfcc_ref.py restates them in fp64 NumPy and the kernels are held against
 * that.  Dither is not supported (this is the --dither=0 program).  No floating-point atomics, no cross-workgroup hand-over: the output
 * bits depend on the shape of the call only.
 *
 * With sf = sample_frequency: L = (int)(sf * 0.001 * frame_length_ms) samples per frame, S the same of frame_shift_ms, N the smallest
 * power of two >= L; N must be 128, 256, 512 or 1024.  An utterance of n int16 samples (used as floats, unscaled) has
 *   T = snip_edges ? (n < L ? 0 : 1 + (n - L) / S) : (n + S / 2) / S   frames (integer division); frame f starts at sample
 *   snip_edges ? f * S : S * f + S / 2 - L / 2; an index i outside [0, n) is replaced by -i - 1 (i < 0) or 2 n - 1 - i until it is inside.
 * Per frame: subtract sum / L (remove_dc_offset); logE = log(max(sum w^2, FLT_EPSILON)) (raw_energy); w[i] -= p w[i - 1] for i = L - 1 ..
 * 1, w[0] -= p w[0]; multiply by the Povey window (0.5 - 0.5 cos(2 pi i / (L - 1)))^0.85; logE by the same formula here when raw_energy
 * is off; zero-pad to N, real FFT, P[k] = |X[k]|^2; mel energies E[m] = sum_k W[m][k] P[k] over k < N / 2 (the Nyquist bin is not used)
 * with mel(f) = 1127 ln(1 + f / 700), bin m's left / centre / right at mel(low) + (m, m + 1, m + 2) (mel(high) - mel(low)) / (bins + 1),
 * W non-zero only where left < mel(k sf / N) < right: (mel - left) / (centre - left) if mel <= centre else (right - mel) / (right -
 * centre); logmel = log(max(E, FLT_EPSILON)); DCT-II (row 0 sqrt(1 / bins), row c sqrt(2 / bins) cos(pi / bins (m + 0.5) c)), first
 * num_ceps rows, times the lifter 1 + 0.5 Q sin(pi c / Q) (Q = cepstral_lifter, 0 = none); use_energy: coefficient 0 = logE, floored
 * at log(energy_floor) when energy_floor > 0. */
typedef struct xv_mfcc_config {
    int32_t struct_bytes;             /* = sizeof(xv_mfcc_config) of the header the host was built against; anything else is refused */
    float sample_frequency;           /* 16000 */
    float frame_length_ms;            /* 25 */
    float frame_shift_ms;             /* 10 */
    int32_t num_mel_bins;             /* 30; <= 128 */
    int32_t num_ceps;                 /* 30; <= num_mel_bins */
    float low_freq;                   /* 20 */
    float high_freq;                  /* 7600; <= 0: the Nyquist frequency plus this value */
    int32_t snip_edges;               /* 0 (the VoxCeleb conf sets false; Kaldi's own default is true) */
    float preemphasis;                /* 0.97 */
    int32_t remove_dc_offset;         /* 1 */
    float cepstral_lifter;            /* 22 */
    int32_t use_energy;               /* 1 */
    int32_t raw_energy;               /* 1 */
    float energy_floor;               /* 0 */
} xv_mfcc_config;
/* T of an utterance of `samples` samples; -1 (xv_last_error) for a configuration that is refused.  Host arithmetic. */
int64_t xv_mfcc_num_frames(const xv_mfcc_config* cfg, int64_t samples);
/* The constant tables of xv_mfcc, computed in double and rounded to fp32 once - host arithmetic, no GPU call: a C host builds them
 * without Python and copies them to the device.  xv_mfcc_table_floats: their size (0 for a refused configuration); xv_mfcc_tables
 * writes them into host_out (`floats` must be that size).  Layout, in floats, one block behind the other:
 *   window   [L]            the Povey window
 *   twiddles [N / 2][2]     (cos, -sin)(2 pi k / N), k < N / 2
 *   mel_bins [bins][3]      per mel bin: the first FFT bin with a non-zero weight, how many consecutive FFT bins have one, the offset
 *                           of the bin's weights in the next block (whole numbers stored as floats; an empty bin is 0, 0, its offset)
 *   mel_w    [sum of counts] the non-zero weights, bin after bin
 *   dct      [num_ceps][bins] DCT row c times the lifter of c */
size_t xv_mfcc_table_floats(const xv_mfcc_config* cfg);
int xv_mfcc_tables(const xv_mfcc_config* cfg, float* h_out, size_t floats);
/* out[i][f][:] = the MFCC of frame f of utterance i for f < rows_out[i] = min(T_i, t_out), zero rows behind - fp32 [b][t_out][num_ceps],
 * the layout xv_cm_decode_ragged leaves, so xv_frontend and xv_engine_forward_lengths take it as it is.  pcm: device int16, the samples
 * of all utterances back to back; utterance i starts at sample offsets[i] (device int64 [b], any 2-byte alignment) and has samples[i]
 * samples (device int32 [b]; <= 0: no frame) - the caller guarantees that every [offsets[i], offsets[i] + samples[i]) lies inside the
 * buffer (ops.mfcc checks the host arrays before the upload).  tables_dev: what xv_mfcc_tables wrote for the same cfg, on the device.
 * One launch: a wave per frame, four waves walking sixteen frames per workgroup behind one copy of the tables into LDS. */
int xv_mfcc(void* stream, const xv_mfcc_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
            const int32_t* samples, int b, int t_out, float* out, int32_t* rows_out);
/* compute-vad-decision on a padded batch of feature matrices x [b][t][d], piece i holding rows[i] frames (T below; clamped to 0 .. t),
 * e[f] = x[i][f][0]: thr = threshold + mean_scale * mean(e) (the mean summed in double in a fixed order; mean_scale == 0: threshold
 * alone); frame f is voiced iff #{f' in [f - c, f + c] and [0, T) : e[f'] > thr} >= (size of that window) * proportion, c =
 * frames_context.  masks: one byte per frame [b][t], 1 or 0, bytes behind rows[i] zero - the mask form xv_frontend reads, with
 * mask_offsets[i] = i * t.  rows: device int32 [b].  One workgroup per piece.  The VoxCeleb vad.conf: 5.5, 0.5, 2, 0.12. */
int xv_energy_vad(void* stream, const float* x, const int32_t* rows, int b, int t, int d, float threshold, float mean_scale,
                  int frames_context, float proportion, uint8_t* masks);

/* Log-mel filterbank energies from waveforms: compute-fbank-feats with --dither=0, which is compute-mfcc-feats stopped in front of the
 * DCT.  Parity is BY RESTATEMENT, as for xv_mfcc: the rules are the specification, tests/fbank_ref.py restates them in fp64 on top of
 * tests/mfcc_ref.py, the kernel is held against that.  The same kernel body runs both feature kinds; no floating-point atomics, the
 * output bits depend on the shape of the call only.
 *
 * L, S, N, T, the frame's first sample, the reflection, the DC removal, logE (raw_energy: in front of the pre-emphasis, otherwise
 * behind the window), the pre-emphasis, the Povey window, the FFT and the mel energies E[m] are xv_mfcc's, word for word (above), but
 * for P[k]: use_power ? |X[k]|^2 : sqrtf(|X[k]|^2).  Then column m of a frame is use_log_fbank ? log(max(E[m], FLT_EPSILON)) : E[m];
 * with use_energy, column 0 is logE, floored at log(energy_floor) when energy_floor > 0, and the mel columns follow it:
 * d = num_mel_bins + use_energy floats per frame, d <= 128 (what xv_frontend and xv_cm_encode take; more is refused by name). */
typedef struct xv_fbank_config {
    int32_t struct_bytes;             /* = sizeof(xv_fbank_config) of the header the host was built against; anything else is refused */
    float sample_frequency;           /* 16000 */
    float frame_length_ms;            /* 25 */
    float frame_shift_ms;             /* 10 */
    int32_t num_mel_bins;             /* 23 (compute-fbank-feats' own defaults throughout); <= 128 */
    float low_freq;                   /* 20 */
    float high_freq;                  /* 0; <= 0: the Nyquist frequency plus this value */
    int32_t snip_edges;               /* 1 */
    float preemphasis;                /* 0.97 */
    int32_t remove_dc_offset;         /* 1 */
    int32_t use_energy;               /* 0 */
    int32_t raw_energy;               /* 1 */
    float energy_floor;               /* 0 */
    int32_t use_log_fbank;            /* 1 */
    int32_t use_power;                /* 1 */
} xv_fbank_config;
/* T of an utterance of `samples` samples (xv_mfcc_num_frames' rule); -1 (xv_last_error) for a configuration that is refused.  Host
 * arithmetic. */
int64_t xv_fbank_num_frames(const xv_fbank_config* cfg, int64_t samples);
/* The constant tables of xv_fbank - host arithmetic, no GPU call: the layout of xv_mfcc_tables without its last block (window [L],
 * twiddles [N / 2][2], mel_bins [bins][3], mel_w [sum of counts]), the same numbers for the same fields.  xv_fbank_table_floats: their
 * size (0 for a refused configuration); xv_fbank_tables writes them into h_out (`floats` must be that size). */
size_t xv_fbank_table_floats(const xv_fbank_config* cfg);
int xv_fbank_tables(const xv_fbank_config* cfg, float* h_out, size_t floats);
/* out[i][f][:] = the d columns of frame f of utterance i for f < rows_out[i] = min(T_i, t_out), zero rows behind - fp32 [b][t_out][d],
 * the layout xv_mfcc leaves: xv_frontend, xv_cm_encode and xv_engine_forward_lengths take it as it is.  pcm, offsets, samples: as for
 * xv_mfcc, the caller guaranteeing the ranges (ops.fbank checks the host arrays before the upload).  tables_dev: what xv_fbank_tables
 * wrote for the same cfg, on the device.  energy_out: NULL, or fp32 [b][t_out]: logE of every frame by the rule above, floor included
 * (zeros behind rows_out[i]), WHATEVER use_energy says - with the options of an xv_mfcc_config it holds the bits of that call's column
 * 0, so xv_energy_vad(x = energy_out, d = 1) gives the decisions an MFCC pass with use_energy gives: the second feature pass Kaldi
 * recipes run for the VAD of an fbank system is not needed.  One launch, xv_mfcc's grid. */
int xv_fbank(void* stream, const xv_fbank_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
             const int32_t* samples, int b, int t_out, float* out, int32_t* rows_out, float* energy_out);

/* Reverberation and additive-noise augmentation of waveforms: what the training list of the recipe pipes through wav-reverberate
 * (egs/voxceleb/v1/run.sh:68-130: the reverberated, noise, music and babble copies of the clean list), with --normalize-output=true as
 * its default.  Kaldi is not available where this project is built and tested: parity is BY RESTATEMENT, as for xv_mfcc - the rules
 * below are the specification ("as restated", not "as Kaldi", wherever the two could differ: DESIGN.md section 6d lists what is
 * unpinned), tests/augment_ref.py restates them in fp64 and the kernels are held against that.
 *
 * One output utterance: source x (int16, n >= 1 samples, used as floats, unscaled), optional impulse response h (int16, L >= 1 taps,
 * unscaled), noises j = 0 .. J - 1 in list order (int16 v_j of len_j samples, snr_j dB, start sample o_j >= 0, span m_j >= 1).
 *   1. P0 = sum x^2 / n.
 *   2. With h: p = the first index of max(h); the early part is h[es:ee], es = max(p - trunc(0.001f * fs), 0), ee = min(p + trunc(0.05f
 *      * fs), L), the products taken in fp32 by the host, which passes es, ee and p in the tables; E = sum (x * h[es:ee])^2 / (n + (ee - es) - 1), the mean
 *      square of the FULL convolution over its whole length; y = x * h, M = n + L - 1 samples.
 *   3. Without h: E = P0, y = x, M = n, p = 0.
 *   4. Noise j is v_j[i mod len_j] for i < m_j (m_j = len_j: a foreground noise, added once at o_j; m_j = M with o_j = 0: the background
 *      form, the noise repeated over the utterance).  Pn_j = sum_{i < m_j} v_j[i mod len_j]^2 / m_j, g_j = sqrt(10^(-snr_j / 10) * E /
 *      Pn_j), y[o_j + i] += g_j * v_j[i mod len_j] for i < min(m_j, M - o_j).  A noise with Pn_j = 0 or o_j >= M adds nothing.
 *   5. Pa = sum y^2 / M.  s = (normalize_output && Pa > 0 ? sqrt(P0 / Pa) : 1) * (volume > 0 ? volume : 1); y *= s.
 *   6. out[i] = y[(i + shift) mod M] for i < n_out; shift_output: shift = p, n_out = n; otherwise shift = 0, n_out = M.
 *   7. PCM-16: truncate toward zero, then clamp to [-32768, 32767].
 * Numerics: P0, E, Pn_j and Pa are summed in double in a fixed order, no floating-point atomics; g_j and s are computed in double and
 * rounded to fp32 once; the convolution, the additions of step 4 and the product of step 5 run in fp32, the first two with one fma per
 * term.  The convolution is a direct-form FIR: taps in blocks of XV_AUG_KB anchored at tap 0, a block summed sequentially from zero in
 * tap order, the block sums added sequentially in block order - the longest add chain of an output is chain(L) = XV_AUG_KB +
 * ceil(L / XV_AUG_KB) roundings, never one chain over all L taps.  The output bits depend on the shape of the call only. */
#define XV_AUG_TILE 1024              /* consecutive outputs of one utterance per workgroup */
#define XV_AUG_KB 32                  /* taps per block of the add chain */
typedef struct xv_augment_config {
    int32_t struct_bytes;             /* = sizeof(xv_augment_config) of the header the host was built against; anything else is refused */
    float sample_frequency;           /* 16000; enters es / ee only, which the host computes: carried so that one struct says it all */
    int32_t shift_output;             /* 1 (the recipe's setting) */
    int32_t normalize_output;         /* 1 */
    float volume;                     /* 0: none */
} xv_augment_config;
/* Diagnostics: the plan of one utterance of n samples under L taps (L = 0: no impulse response): out[0] tiles = ceil(M / XV_AUG_TILE),
 * out[1] XV_AUG_TILE, out[2] XV_AUG_KB, out[3] chain(L) (0 for L = 0).  Host arithmetic, nothing is launched. */
int xv_debug_augment_plan(int64_t n, int64_t L, int out[4]);
/* Bytes of workspace of an xv_augment call over b utterances with n_entries noise entries and n_tiles tiles in all (the sum of the plan's
 * tiles): y in fp32, a tile's XV_AUG_TILE samples at its index, and one double per tile for each of E and Pa, per utterance for P0, per
 * entry for Pn.  0 for negative counts.  Host arithmetic. */
size_t xv_augment_workspace_bytes(int b, int n_entries, int64_t n_tiles);
/* The three pools hold int16 samples back to back on the device (rir_pcm / noise_pcm may be NULL when nothing refers to them).  tables:
 * ONE device int64 array - the call's only index upload - of XV_AUG_UTT_WORDS * b + XV_AUG_NOISE_WORDS * n_entries + 2 * n_tiles words:
 *   per utterance i  [b][10]:  source offset, n, rir offset (-1: no impulse response), L, es, ee, p, first noise entry, number of noise
 *                              entries, output offset (in samples, of out_pcm and out_f32 alike)
 *   per noise entry  [n_entries][5]: offset, len, snr (the fp32 bit pattern in the low 32 bits), start o, span m - utterance after
 *                              utterance in list order
 *   per tile         [n_tiles][2]: utterance, first output - for each utterance in order, the ceil(M / XV_AUG_TILE) tiles of its y
 * Nothing in it is checked on the device: the caller guarantees that every range lies inside its pool, 0 <= es < ee <= L, 0 <= p < L,
 * M < 2^31 and that the outputs do not overlap (ops.augment checks the host arrays before the upload, as ops.mfcc does).
 * out_pcm: int16, utterance i's n_out samples at its output offset - the packed layout xv_mfcc reads, with out_samples [b] = n_out as
 * its `samples`; samples between the utterances are not written.  out_f32 (NULL: not wanted): the fp32 values of step 6 at the same
 * offsets.  clipped [b]: how many samples of the utterance the clamp of step 7 changed.
 * Launches: the powers (one workgroup per signal); the FIR in its `energy` role (the early part; one double per tile) and its `store`
 * role (y) - both only when an utterance has an impulse response; mix (noises, one double of sum y^2 per tile); finish (steps 5 - 7).
 * One workgroup per tile in the last four. */
#define XV_AUG_UTT_WORDS 10
#define XV_AUG_NOISE_WORDS 5
int xv_augment(void* stream, const xv_augment_config* cfg, int b, int n_entries, int64_t n_tiles, const int16_t* src_pcm,
               const int16_t* rir_pcm, const int16_t* noise_pcm, const int64_t* tables, size_t table_words, int any_rir, void* ws,
               size_t ws_bytes, int16_t* out_pcm, float* out_f32, int32_t* out_samples, int32_t* clipped);

/* Sample-rate conversion of waveforms: the `sox -r 8k` stages of the 8 kHz recipes (egs/sre/v1/local/make_musan.sh, run.sh:135-142),
 * compute-mfcc-feats --allow-downsample / --allow-upsample, and speed perturbation (a factor F at rate fs is the resample F * fs -> fs,
 * F * fs a whole number: 0.9 at 16 kHz is 14400 -> 16000).  A polyphase windowed-sinc FIR: Kaldi's LinearResample with the cutoff of
 * ResampleWaveform (feat/resample.{h,cc}).  Kaldi is not available where this project is built and tested: parity is BY RESTATEMENT, as
 * for xv_mfcc and xv_augment - the rules below are the specification ("as restated", not "as Kaldi" or "as sox"; DESIGN.md section 6f
 * lists what is unpinned), tests/resample_ref.py restates them in fp64 and the kernel is held against that.
 *
 * Integer rates fin != fout (Hz), num_zeros (6), cutoff (0.99 * 0.5 * min(fin, fout)).  Every table value is computed in DOUBLE and
 * rounded to fp32 once (Kaldi's FilterFunc works in float: a deliberate difference).
 *   g = gcd(fin, fout), in_unit = fin / g, out_unit = fout / g, ww = num_zeros / (2.0 * cutoff).
 *   Phase i < out_unit: t = i / (double)fout, first[i] = ceil((t - ww) * fin), last[i] = floor((t + ww) * fin), taps[i] = last - first + 1.
 *   Weight of input index k = first[i] + j: d = k / (double)fin - t, w[i][j] = filter(d) * window(d) / fin with
 *     window(d) = 0.5 * (1 + cos(2 pi * cutoff / num_zeros * d)) if |d| < ww, else 0;
 *     filter(d) = sin(2 pi * cutoff * d) / (pi * d) if d != 0, else 2 * cutoff.
 *   Rows are padded with zeros to taps_max = max_i taps[i].
 *   n samples give n_out = ceil(n * out_unit / in_unit) (whole numbers; LinearResample's GetNumOutputSamples with flush = true); n <= 0: 0.
 *   Output o: q = o / out_unit, i = o mod out_unit, f = first[i] + q * in_unit, y[o] = sum_j w[i][j] * x[f + j] over the j with
 *   0 <= f + j < n, the int16 samples used as floats, unscaled.  The sum is ONE sequential chain of fmaf from zero in increasing j, at
 *   most taps_max long: the bits of y depend on x and the table only - not on the tile, the batch or the launch.
 *   PCM-16: rintf (to nearest, ties to even), then a clamp to [-32768, 32767]; clamped samples are counted per utterance.  (To nearest,
 *   not xv_augment's truncation: this stands where the recipe has a sox stage that writes a wav.)
 * Refused by name on the host, before any launch: fin == fout (callers skip the call), rates < 1, out_unit * taps_max > 16384 floats
 * (the table lives in LDS beside the staged samples: 16000 -> 15999 has 15 999 phases), a table and staging area beyond 128 KiB. */
typedef struct xv_resample_config {
    int32_t struct_bytes;             /* = sizeof(xv_resample_config) of the header the host was built against; anything else is refused */
    int32_t fin;                      /* Hz, >= 1 */
    int32_t fout;                     /* Hz, >= 1, != fin */
    int32_t num_zeros;                /* 0: the default, 6 */
    float cutoff;                     /* Hz; 0: the default, 0.99 * 0.5 * min(fin, fout), formed in double */
} xv_resample_config;
/* n_out of an utterance of `samples` samples; -1 (xv_last_error) for a configuration that is refused.  Host arithmetic. */
int64_t xv_resample_num_samples(const xv_resample_config* cfg, int64_t samples);
/* The constant table of xv_resample - host arithmetic, no GPU call.  xv_resample_table_floats: its size (0 for a refused
 * configuration); xv_resample_tables writes it into host_out (`floats` must be that size).  Layout, in floats:
 *   first [out_unit]              first[i]  (whole numbers stored as floats, like xv_mfcc's mel_bins)
 *   taps  [out_unit]              taps[i]
 *   w     [out_unit][taps_max]    the weight rows, zeros behind taps[i] */
size_t xv_resample_table_floats(const xv_resample_config* cfg);
int xv_resample_tables(const xv_resample_config* cfg, float* host_out, size_t floats);
/* Diagnostics: out[0] in_unit, out[1] out_unit, out[2] taps_max, out[3] consecutive outputs of one utterance per tile, out[4] input
 * samples staged per tile (tile * in_unit / out_unit + taps_max, rounded up to whole periods), out[5] bytes of dynamic LDS of a
 * workgroup (weight rows on an odd pitch, first[], the staged samples).  Host arithmetic, nothing is launched. */
int xv_debug_resample_plan(const xv_resample_config* cfg, int out[6]);
/* pcm: device int16, the samples of all utterances back to back; utterance i starts at sample offsets[i] (device int64 [b], any 2-byte
 * alignment) and has samples[i] samples (device int32 [b]; <= 0: no output) - the layout xv_mfcc and xv_augment read.  tables_dev: what
 * xv_resample_tables wrote for the same cfg, on the device.  out_pcm: int16, utterance i's n_out samples at out_offsets[i] (device int64
 * [b]) - the packed layout xv_mfcc reads, with out_samples [b] = n_out as its `samples`; samples between the utterances are not written.
 * out_f32 (NULL: not wanted): y before the rounding, at the same offsets.  clipped [b]: how many samples of the utterance the clamp
 * changed.  Nothing is checked on the device: the caller guarantees that every range lies inside its buffer, that n_out < 2^31 and that
 * the outputs do not overlap (ops.resample checks the host arrays before the upload).  b <= 65535.
 * One launch: a workgroup copies the table into LDS once and walks tiles of one utterance; per tile the input span is staged as fp32
 * with zeros outside [0, n). */
int xv_resample(void* stream, const xv_resample_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
                const int32_t* samples, int b, const int64_t* out_offsets, int16_t* out_pcm, float* out_f32, int32_t* out_samples,
                int32_t* clipped);

/* Cosine trial scoring with adaptive symmetric score normalisation (AS-norm) on embedding matrices: the stage behind extract.py, for
 * which the reference recipe goes to Kaldi (ivector-mean | ivector-subtract-global-mean | ivector-normalize-length, then
 * ivector-compute-dot-products; egs/voxceleb/v1/run.sh, cosine back end).  All arrays on the device, pitches in floats.  No
 * floating-point atomics, no cross-workgroup hand-over: the output bits depend on the shape of the call only.
 *
 * Row sums of the first two ops: one wave per row; a lane's partial takes the elements lane, lane + 64, ... (groups of four when d,
 * the pitches and the bases are multiples of 4 floats / 16 bytes, single elements otherwise) with one fma each, a six-step butterfly
 * adds the lanes.  The longest add chain is chain(d) = 4 * ceil(d / 256) + 6 roundings in either form.
 *
 * score_prepare: y[r][c] = v[c] * rsqrt(max(sum_c v[c]^2, 1e-12)) with v[c] = x[r][c] - mean[c] (mean = NULL: v = x) for c < d - the
 * epsilon rule of xv_l2_scaling_forward - and y[r][c] = 0 for d <= c < ldy, in every row (y holds rows * ldy floats), so y is a GEMM
 * operand as it stands.  A zero row gives a zero row.  In place (y == x and ldy == ldx) is allowed; any other overlap of x or mean
 * with y is refused. */
int xv_score_prepare(void* stream, const float* x, int rows, int d, int ldx, const float* mean, float* y, int ldy);
/* score_trials: s = sum_{c<d} e[ei[j]][c] * t[ti[j]][c] for j < m.  e_stats == t_stats == NULL: out[j] = s.  Both given ([ne][2] and
 * [nt][2]: mean, deviation of each row's cohort scores, from xv_score_cohort_stats): out[j] = 0.5 * ((s - e_stats[ei[j]][0]) /
 * e_stats[ei[j]][1] + (s - t_stats[ti[j]][0]) / t_stats[ti[j]][1]).  One of the two alone is refused.  ei, ti: device int32 [m];
 * they are NOT checked on the device - the caller guarantees 0 <= ei[j] < ne and 0 <= ti[j] < nt (ops.score_trials checks the host
 * arrays before the upload). */
int xv_score_trials(void* stream, const float* e, int lde, int ne, const float* t, int ldt, int nt, int d, const int32_t* ei,
                    const int32_t* ti, int64_t m, const float* e_stats, const float* t_stats, float* out);
/* score_cohort_stats: stats[r] = (mean, sqrt(max(var, 1e-12))) - var the biased variance, taken around that mean in a second pass -
 * of the k = min(top_k, n_cohort) largest of the scores sum_c x[r][c] * cohort[j][c], j < n_cohort.  The scores come from the fp32 GEMM
 * behind xv_affine_forward (k = 1, segs = rows, t_in = 1, the cohort in the wt[o][c] layout) with K = d rounded up to 4: columns d .. K
 * of both operands are read and must be zero (xv_score_prepare writes them), and the GEMM's own operand rules hold (pitches multiples
 * of 4, 16-byte aligned bases, each operand below 4 GB) - it refuses by name.  It writes a slab [tile][n_cohort rounded up to 4] in ws,
 * tile = the largest multiple of 128 rows ws_bytes holds; rows beyond a tile take further GEMM launches.  xv_score_cohort_workspace_bytes
 * is the size at which one launch covers all rows; a workspace that holds one 128-row tile works, less (or a base off the 16-byte grid)
 * is refused.  Per row one workgroup then selects the k-th largest score exactly (radix select on the order-preserving unsigned key of
 * the float, four 8-bit passes) and sums in double, in a fixed order, the scores strictly above it plus (k - their count) copies of it -
 * a cut through a run of equal scores is well defined - and the squared distances to the mean the same way.  top_k <= 0 and
 * n_cohort <= 0 are refused. */
size_t xv_score_cohort_workspace_bytes(int rows, int n_cohort, int d);
int xv_score_cohort_stats(void* stream, const float* x, int ldx, int rows, const float* cohort, int ldc, int n_cohort, int d, int top_k,
                          float* stats, void* ws, size_t ws_bytes);
/* score_normalize (the AS-norm of scores that are on the device already: the PLDA log-likelihood ratios of egs/sre/v1/run.sh:477-490,
 * normalised as score_trials normalises a cosine): out[j] = 0.5 * ((s - e_stats[ei[j]][0]) / e_stats[ei[j]][1] + (s - t_stats[ti[j]][0]) /
 * t_stats[ti[j]][1]), s = scores[j], j < m - the expression of score_trials, compiled once for both, so the same bits for the same s and
 * statistics.  In place (out == scores) is allowed, any other overlap is refused.  ei, ti: device int32 [m], NOT checked on the device
 * (ops.score_normalize checks the host arrays before the upload). */
int xv_score_normalize(void* stream, const float* scores, const int32_t* ei, const int32_t* ti, int64_t m, const float* e_stats,
                       const float* t_stats, float* out);
/* score_dense (the all-pairs matrix of one recording's prepared rows, for the clusterer below): out[i][j] = sum_c x[i][c] * x[j][c],
 * i, j < n, on rows x [n][ldx] prepared by xv_score_prepare or by the back end's unit chain.  One launch of the fp32 GEMM of
 * score_cohort_stats (the rows on both sides, K = d rounded up to 4: columns d .. K are read and must be zero, pitch a multiple of 4,
 * 16-byte aligned base, below 4 GB - the GEMM refuses by name), written straight into out [n][ldo]: ldo >= n, any alignment, so out may be
 * a view into a packed buffer of many recordings; columns n .. ldo are not written.  out[i][j] and out[j][i] come from different lanes of
 * the GEMM's tile and are not promised to be the same bits: xv_ahc_cluster reads the upper triangle only. */
int xv_score_dense(void* stream, const float* x, int ldx, int n, int d, float* out, int ldo);

/* The LDA / PLDA back end behind extraction, device side: what ivector-mean (with and without spk2utt), ivector-compute-lda,
 * ivector-compute-plda, ivector-subtract-global-mean and ivector-plda-scoring --normalize-length=true do on the embedding tables
 * (egs/voxceleb/v1/run.sh:370-401, egs/sre/v1/run.sh:397-490).  The eigendecompositions and the EM of the two estimators run on the host
 * in fp64 (misc/backend.py); the affine maps A v + b and offset + transform y are xv_affine_forward (k = 1, bias = the offset).  All
 * arrays on the device, pitches in floats.  No floating-point atomics, no cross-workgroup hand-over: the output bits depend on the shape
 * of the call only.  d <= 0 is refused by every op.
 *
 * group_means (ivector-mean ark:spk2utt, and the per-speaker averages of both estimators): group g lists the rows
 * rows[offsets[g] .. offsets[g + 1]) of x [n][ldx] (CSR: offsets int64 [groups + 1], offsets[0] = 0, offsets[groups] = total; rows int32
 * [total]; a row may be listed more than once and in any order).  mean64[g][c] = the sum of the listed rows, added in list order in
 * double, divided by their count - IEEE adds and one IEEE divide, so the bits are defined by the list; mean32 (optional) [groups][ldm] =
 * its fp32 rounding, columns d .. ldm zero.  One thread per (group, column).  groups <= 0 and total < groups (some group would be
 * empty) are refused; offsets and rows are NOT checked on the device - the caller guarantees non-empty groups and 0 <= rows[i] < n
 * (ops.backend_group_means checks the host arrays before the upload and refuses an empty group by name). */
int xv_backend_group_means(void* stream, const float* x, int n, int ldx, int d, const int64_t* offsets, const int32_t* rows, int groups,
                           int64_t total, double* mean64, float* mean32, int ldm);
/* center (ivector-subtract-global-mean alone, the input of the LDA): y[r][c] = x[r][c] - mean[c] in fp32 (mean = NULL: a copy) for
 * c < d, 0 for d <= c < ldy in every row, so y is a GEMM operand as it stands.  In place (y == x and ldy == ldx) is allowed; any other
 * overlap of x or mean with y is refused. */
int xv_backend_center(void* stream, const float* x, int rows, int d, int ldx, const float* mean, float* y, int ldy);
/* scatter (the statistics of ivector-compute-lda / ivector-compute-plda): c64 [d][d] (double) = sum_r v_r v_r^T over the rows of
 * x [n][ldx], v = x[r] - mean in fp32 as score_prepare subtracts it (mean = NULL: v = x[r]).  The rows are taken in blocks of 8 192; a
 * block's products come from the fp32 TN GEMM behind xv_affine_wgrad (k = 1, segs = rows, t_in = 1, the block on both sides, M = N = d
 * rounded up to 4), which writes its split slabs into ws; one more kernel adds the slabs into c64 in slab order, block after block, in
 * double, one thread per element - so no fp32 add chain is longer than the reduction rows of one GEMM workgroup (out[2] of
 * xv_debug_tn_plan(d4, d4, block rows, 0, out)), whatever n is.  An element (i, j) is read from the upper triangle of the slabs:
 * c64 is bit-symmetric.  A block is first copied into ws (centred, padding columns zeroed) unless it is a GEMM operand as it stands (no
 * mean, d and ldx multiples of 4, 16-byte aligned base); the copy is exact.  ws: xv_backend_scatter_workspace_bytes(n, d) bytes, 16-byte
 * aligned - fewer (less than the centred block plus the slabs) is refused, and the GEMM refuses by name what it refuses. */
size_t xv_backend_scatter_workspace_bytes(int n, int d);
int xv_backend_scatter(void* stream, const float* x, int n, int d, int ldx, const float* mean, double* c64, void* ws, size_t ws_bytes);
/* plda_normalize (Plda::TransformIvector, normalize_length = true, simple_length_norm = false): out[r][c] = u[r][c] * sqrt(d / s_r),
 * s_r = sum_c u[r][c]^2 / (psi[c] + 1 / n_utts[r]) (n_utts = NULL: 1 everywhere) for c < d, 0 for d <= c < ldo.  One wave per row, the
 * lanes and the chain(d) of score_prepare.  A row whose sum is 0 stays 0.  In place (out == u and ldo == ldu) is allowed; any other
 * overlap of u or psi with out is refused. */
int xv_backend_plda_normalize(void* stream, const float* u, int rows, int d, int ldu, const float* psi, const int32_t* n_utts, float* out,
                              int ldo);
/* plda_trials (Plda::LogLikelihoodRatio): out[j] = k0[q] + sum_{c<d} (-0.5 iv[q][c] (t_c - a[q][c] e_c)^2 + 0.5 g[c] t_c^2), e = row ei[j] of
 * e [ne][lde], t = row ti[j] of t [nt][ldt], q = nidx[ei[j]] the enrol row's entry in the table of distinct utterance counts:
 * coef [n_distinct][2][ldc] = (a = n psi / (n psi + 1), iv = 1 / (1 + psi / (n psi + 1))), g[c] = 1 / (psi[c] + 1), k0[q] = -0.5 sum log v +
 * 0.5 sum log(psi + 1), all built on the host in double and rounded once (misc/backend.py plda_coefficients): no division and no
 * logarithm on the device.  One wave per trial; the two quadratic forms are one interleaved sum per lane.  ei, ti [m], nidx [ne]: device
 * int32, NOT checked on the device - the caller guarantees 0 <= ei[j] < ne, 0 <= ti[j] < nt, 0 <= nidx[i] < n_distinct
 * (ops.backend_plda_trials checks the host arrays before the upload). */
int xv_backend_plda_trials(void* stream, const float* e, int lde, int ne, const float* t, int ldt, int nt, int d, const int32_t* ei,
                           const int32_t* ti, int64_t m, const int32_t* nidx, const float* coef, int ldc, int n_distinct, const float* g,
                           const float* k0, float* out);
/* plda_cohort_stats (the cohort statistics of AS-norm behind the PLDA scores of egs/sre/v1/run.sh:477-490): stats[r] = (mean,
 * sqrt(max(var, 1e-12))) of the k = min(top_k, n_cohort) largest log-likelihood ratios of row r of x [rows][ldx] - a PLDA-normalised row
 * in the model role, q = nidx[r] its entry in the table of distinct utterance counts (nidx = NULL: 0 for every row) - against the rows of
 * cohort [n_cohort][ldc], normalised with one utterance, in the test role.  coef, g, k0: the tables of plda_trials.  The ratio is taken
 * in its factored form LLR(e, t) = R(e) + C_q(t) + sum_c (iv_q[c] a_q[c] e_c) t_c with R(e) = k0[q] - 0.5 sum_c iv_q[c] a_q[c]^2 e_c^2 and
 * C_q(t) = 0.5 sum_c (g[c] - iv_q[c]) t_c^2: one kernel writes C_q(t_j) for every (q, j), once per call; per tile of rows one kernel
 * writes the GEMM operand xs = (iv a) x on the pitch d rounded up to 4 (zero padding) and R, the fp32 GEMM of score_cohort_stats writes
 * xs . cohort^T into the slab, and the selection of score_cohort_stats - the same code - runs over v(r, j) = (slab[r][j] + C_q[j]) +
 * R[r], two plain fp32 adds.  For n = 1 the ratio is symmetric in (e, t), so a test row is passed as a one-utterance model.  ws, in
 * floats: [n_distinct][P] column terms, then per round [tile][P] slab, [tile][K] operand, [tile] row terms, P = n_cohort and K = d rounded
 * up to 4, tile = the largest multiple of 128 rows ws_bytes holds; xv_backend_plda_cohort_workspace_bytes is the size at which one round
 * covers all rows.  Refused by name: top_k <= 0, n_cohort <= 0, d <= 0, ldx or ldc below d rounded up to 4 (columns d .. K of the cohort
 * rows are read and must be zero: plda_normalize writes them), ldcoef below d, a workspace below the column terms plus one 128-row tile or
 * off the 16-byte grid, and what the GEMM refuses.  nidx is NOT checked on the device (ops.backend_plda_cohort_stats checks the host array). */
size_t xv_backend_plda_cohort_workspace_bytes(int rows, int n_cohort, int d, int n_distinct);
int xv_backend_plda_cohort_stats(void* stream, const float* x, int ldx, int rows, const int32_t* nidx, const float* cohort, int ldc,
                                 int n_cohort, int d, const float* coef, int ldcoef, int n_distinct, const float* g, const float* k0,
                                 int top_k, float* stats, void* ws, size_t ws_bytes);
/* plda_dense (ivector-plda-scoring-dense behind its per-recording PCA, which is xv_backend_pca_plda below: with that op's map, psi and tables
 * the recipe's scores under --target-energy, with the global model's the scores without it; the all-pairs matrix of one recording, for the clusterer):
 * out[r][j] = the one-utterance log-likelihood ratio of rows r and j of x [n][ldx] (PLDA-normalised with one utterance), in the factored
 * form of plda_cohort_stats with the single table entry of n_utts = 1 (coef [2][ldk], g, k0 [1]): out[r][j] = (slab[r][j] + C[j]) + R[r].
 * The column-term and fold kernels and the GEMM are plda_cohort_stats' (the rows are their own cohort); the GEMM writes the slab into out
 * and one small kernel adds the two terms in place, so the error budget of an element is plda_cohort_stats'.  out [n][ldo]: ldo >= n, any
 * alignment (a view into a packed buffer); columns n .. ldo are not written.  The result is not bit-symmetric (the GEMM's operands differ
 * by the fold; the two adds are taken in the order above): xv_ahc_cluster reads the upper triangle only.  ws, in floats: [P] column terms,
 * [n][K] folded rows, [n] row terms, P = n and K = d rounded up to 4; xv_backend_plda_dense_workspace_bytes(n, d) bytes, 16-byte aligned -
 * fewer is refused, as are n <= 0, d <= 0, ldx below K, ldk below d, ldo below n and what the GEMM refuses. */
size_t xv_backend_plda_dense_workspace_bytes(int n, int d);
int xv_backend_plda_dense(void* stream, const float* x, int ldx, int n, int d, const float* coef, int ldk, const float* g, const float* k0,
                          float* out, int ldo, void* ws, size_t ws_bytes);

/* Agglomerative clustering of score matrices, average linkage on scores (speaker diarization: agglomerative-cluster of Kaldi's
 * callhome_diarization recipes, restated - agreement with a Kaldi run is not pinned).  b recordings per call, one workgroup each, no
 * hand-over between workgroups: a recording's result depends on its own matrix only and is the same bits every time.
 * Inputs, all on the device: scores, a packed fp32 buffer of scores_floats floats; recording r's matrix [n[r]][ld[r]] starts at float
 * mat_offsets[r] (int64) and only its upper triangle s[i][j], i < j, is read; it is not modified.  targets[r] = 0: stop by threshold;
 * t >= 1: stop at t clusters and ignore the threshold.
 * The arithmetic is part of the operation - a float32 restatement gives the same bits (tests/ahc_ref.py):
 *   clusters start as the singletons 0 .. n - 1, T[i][j] = T[j][i] = s[min(i,j)][max(i,j)], A(a, b) = T[a][b] / (float)(size_a * size_b)
 *   (one correctly rounded fp32 divide).  Step: among the active pairs a < b the largest A, on a tie the lowest a, then the lowest b.
 *   Stop if the cluster count equals max(target, 1); with target = 0 stop unless A >= threshold.  Merge: b goes into a - for every other
 *   active k, T[a][k] = T[k][a] = T[a][k] + T[b][k] (one fp32 add), then size_a += size_b and b is inactive; (a, b, A) is logged.
 * A cluster's id is its smallest member; labels number the final clusters 0, 1, ... in ascending id.  A NaN score is undefined.
 * Outputs: labels int32 [total_n], recording r's at the exclusive prefix of n; merges int32 [total_n - b][2] and merge_values fp32
 * [total_n - b], recording r's log at the exclusive prefix of n - 1, of which the first n_merges[r] entries are written; n_merges int32 [b].
 * total_n = sum n, sum_n2 = sum n^2, max_n = the largest n: host values the caller states.  ws: xv_ahc_workspace_bytes(sum_n2) bytes (T
 * of every recording, full symmetric storage).  Refused by name: b <= 0, max_n < 1, max_n > 2048 (longer recordings take Kaldi's two-pass
 * clustering: xv_ahc_cluster_from and xv_ahc_cluster_sums below), totals that do not fit, a workspace too small.  The device arrays are NOT checked on the host side of this call
 * (ops.ahc_cluster checks the host arrays before the upload: n in 1 .. 2048, ld >= n, 0 <= target <= n, every matrix inside the buffer); a
 * recording whose entries would take the kernel outside the buffers of the call is skipped and gets n_merges = -1. */
size_t xv_ahc_workspace_bytes(int64_t sum_n2);
int xv_ahc_cluster(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n, const int32_t* ld,
                   const int32_t* targets, int b, int max_n, int64_t total_n, int64_t sum_n2, float threshold, int32_t* labels,
                   int32_t* merges, float* merge_values, int32_t* n_merges, void* ws, size_t ws_bytes);

/* The clusterer with a floor and two starts: the two stages of the two-pass clustering of long recordings (Kaldi's
 * AgglomerativeClusterer::ClusterTwoPass behind agglomerative-cluster --first-pass-max-points, as recalled from agglomerative-clustering.cc
 * and restated: contiguous subsets clustered down to ten times the wanted number of clusters, then the survivors against each other;
 * nothing is compared with a Kaldi run, and Kaldi's max_spk_fraction is left out).  The arithmetic, the ties, the merge log, the labels,
 * the layout of every output and the kernel body are xv_ahc_cluster's; tests/ahc2_ref.py restates what differs:
 *   stop rule: recording r merges while its cluster count > floors[r] AND the best A >= threshold (one float per call; -inf: down to the
 *   floor).  floors[r] lies in 1 .. n[r].
 *   seeded = 0, from scores: T from the upper triangle of recording r's matrix at mat_offsets[r] / ld[r], every size 1 - a sub-block of a
 *   larger matrix is a matrix at an offset on the larger one's pitch.  sizes is not read.
 *   seeded = 1: recording r starts from n[r] clusters of sizes int32 [total_n] (recording r's at the exclusive prefix of n, each >= 1,
 *   together at most 32768) and from T [n[r]][n[r]], full symmetric storage at pitch n[r], which the caller has left in ws at the exclusive
 *   prefix of n^2 (xv_ahc_cluster_sums writes sizes and T in this layout); ws is modified.  scores, mat_offsets and ld are not read.
 *   A = T[a][b] / (float)(size_a * size_b): the int32 product may now exceed 2^24; it is exact as an integer (at most 2^28) and converted
 *   to fp32 once, round to nearest even, before the one fp32 divide.
 * ws: xv_ahc_cluster_from_workspace_bytes(sum_n2) bytes.  Refused by name: what xv_ahc_cluster refuses, a seeded other than 0 / 1, a NaN
 * threshold, a missing array of the chosen start.  The device arrays are NOT checked on the host side (ops.ahc_cluster_from checks the host
 * arrays); a recording whose entries would take the kernel outside the buffers of the call, whose floor is outside 1 .. n or whose seeded
 * sizes are wrong is skipped and gets n_merges = -1. */
size_t xv_ahc_cluster_from_workspace_bytes(int64_t sum_n2);
int xv_ahc_cluster_from(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n,
                        const int32_t* ld, const int32_t* floors, const int32_t* sizes, int seeded, int b, int max_n, int64_t total_n,
                        int64_t sum_n2, float threshold, int32_t* labels, int32_t* merges, float* merge_values, int32_t* n_merges, void* ws,
                        size_t ws_bytes);

/* Cluster sums: the seed of the second pass from a recording's score matrix and its first-pass clusters.  b recordings per call; three
 * launches in stream order, no atomics, no wait on another workgroup: the same bits every time.
 * Inputs, all on the device: scores / scores_floats / mat_offsets / n / ld as for xv_ahc_cluster, n[r] in 1 .. 32768, only the upper
 * triangle is read (e(i, j) = s[min(i,j)][max(i,j)], the diagonal is not read either); c int32 [b], recording r's clusters, 1 .. min(n[r],
 * 2048); the clusters as member lists: members int32 [total_n], recording r's at the exclusive prefix of n - the rows 0 .. n[r] - 1 cluster
 * by cluster, clusters ascending by their smallest member, a cluster's members ascending; starts int32 [total_c + b], recording r's
 * c[r] + 1 entries at the exclusive prefix of c + 1: cluster B's members are members[starts[B] .. starts[B + 1]), starts[0] = 0,
 * starts[c[r]] = n[r].
 * The order of every sum is part of the operation (tests/ahc2_ref.py restates it with np.cumsum), for clusters A < B:
 *   r_i[B] = the sequential double sum over the members j of B, ascending, of e(i, j)
 *   T[A][B] = T[B][A] = fp32(the sequential double sum over the members i of A, ascending, of r_i[B]);  T[A][A] = 0
 * (a sum starts from its first term, not from 0.0; a fp32 score enters a double sum exactly).
 * Outputs: seed fp32 [sum_c2], recording r's T [c[r]][c[r]] at the exclusive prefix of c^2; sizes int32 [total_c], recording r's at the
 * exclusive prefix of c: what xv_ahc_cluster_from takes as ws and sizes with n = c; status int32 [b]: 0, or -1 for a recording whose
 * entries would take the kernels outside the buffers of the call (spans against the totals, starts not ascending from 0 to n, a member
 * outside 0 .. n - 1): it is skipped.
 * total_n = sum n, total_c = sum c, sum_c2 = sum c^2, sum_nc = sum n c, max_n, max_c: host values the caller states.  ws:
 * xv_ahc_cluster_sums_workspace_bytes(b, sum_nc) bytes, 8-byte aligned (r_i[B] of every recording in double, and the prefixes).  Refused by
 * name: b outside 1 .. 65535, max_n outside 1 .. 32768, max_c outside 1 .. min(max_n, 2048), totals that do not fit, a workspace too
 * small.  The device arrays are NOT checked on the host side of this call (ops.ahc_cluster_sums checks the host arrays: that the lists are
 * a partition in the stated order).  A NaN score is undefined. */
size_t xv_ahc_cluster_sums_workspace_bytes(int b, int64_t sum_nc);
int xv_ahc_cluster_sums(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n,
                        const int32_t* ld, const int32_t* c, const int32_t* members, const int32_t* starts, int b, int max_n, int max_c,
                        int64_t total_n, int64_t total_c, int64_t sum_c2, int64_t sum_nc, float* seed, int32_t* sizes, int32_t* status,
                        void* ws, size_t ws_bytes);

/* Labels at many cuts of one merge log: a threshold changes xv_ahc_cluster's stop rule and nothing else, so the log of a run down to one
 * cluster (every target 1) holds the labels of every threshold as a prefix.  b recordings x cuts cuts per call, one workgroup per
 * (recording, cut), one launch, no hand-over between workgroups; nothing replays sequentially and nothing is floating point behind the
 * comparisons with the threshold: the same bits every time.
 * Inputs, all on the device: the log exactly as xv_ahc_cluster leaves it - merges int32 [total_n - b][2], merge_values fp32 [total_n - b],
 * n_merges int32 [b], n int32 [b] (recording r's entries at the exclusive prefix of n - 1) - and, shared by all recordings, thresholds
 * fp32 [cuts], min_clusters int32 [cuts] (>= 1) and max_clusters int32 [cuts] (>= min_clusters).
 * The rule for cut k of recording r (tests/diar_eval_ref.py restates it):
 *   p = the number of leading log entries with A >= thresholds[k]: it ends at the first entry that fails, not at the count of those that
 *   pass - an fp32 log need not be monotone;
 *   p = min(p, n - min_clusters[k]), then p = max(p, n - max_clusters[k]), either clamped into 0 .. n_merges[r];
 *   the first p merges are applied, b into a: parent[b] = a, independent writes; every row finds its root, and the roots are numbered by
 *   a prefix count - a cluster's id is its smallest member and labels 0, 1, ... follow ascending id, as xv_ahc_cluster numbers them.
 * With min_clusters = 1 and max_clusters >= n the labels are those of xv_ahc_cluster(threshold = thresholds[k]); with min_clusters =
 * max_clusters = t those of xv_ahc_cluster(target = t), bit for bit.
 * Outputs: labels int32 [cuts][total_n], recording r's at the exclusive prefix of n in every cut; clusters int32 [cuts][b], the clusters
 * of each (cut, recording).  A recording with n_merges < 0 or > n - 1, or whose entries lead outside the buffers of the call (n, the
 * totals, an entry without 0 <= a < b < n), and a cut with a NaN threshold or clamps out of order, get clusters = -1 and no labels.
 * Refused by name: b <= 0, max_n outside 1 .. 2048, a total_n that does not fit, cuts outside 1 .. 65535.  The device arrays are NOT
 * checked on the host side of this call (ops.ahc_cut checks the host arrays before the upload and refuses a NaN threshold by name). */
int xv_ahc_cut(void* stream, const int32_t* merges, const float* merge_values, const int32_t* n_merges, const int32_t* n, int b, int max_n,
               int64_t total_n, const float* thresholds, const int32_t* min_clusters, const int32_t* max_clusters, int cuts, int32_t* labels,
               int32_t* clusters);

/* Diarization error counts per (recording, cut): what md-eval counts on 10 ms frames, restated from its definition - nothing is compared
 * with a run of md-eval.  b recordings x cuts label sets per call, one workgroup per (recording, cut), one launch.
 * Inputs, all on the device.  Per recording, for all cuts: ref_mask uint32 [total_frames], bit s set if reference speaker s talks in the
 * frame; scored uint8 [total_frames], 0: the frame is not scored (a collar, ignored overlap); frame_window int32 [total_frames], the window
 * of the recording that owns the frame, or -1; recording r's frames are frame_offsets[r] .. frame_offsets[r + 1] (int64 [b + 1]), its
 * windows' labels lie at win_offsets[r] .. win_offsets[r + 1] (int64 [b + 1]) of a cut's labels; speakers int32 [b], its reference
 * speakers, 1 .. 32 (mask bits at and above are not read).  Per cut: labels int32 [cuts][total_n] (xv_ahc_cut's, or any labels in
 * 0 .. clusters - 1), clusters int32 [cuts][b], out_offsets int64 [cuts][b]: where the block of (cut, recording) starts in overlap.
 * The arithmetic (tests/diar_eval_ref.py restates it), over the scored frames of the recording, h = the label of the frame's window or
 * none, [h] = 1 if there is one, else 0:
 *   speech += popcount(ref);  miss += max(0, popcount(ref) - [h]);  fa += max(0, [h] - popcount(ref));
 *   overlap[s][h] += 1 for every set bit s of ref.
 * Outputs: totals int64 [cuts][b][3] = (speech, miss, fa); overlap int32 [overlap_ints], the block of (cut, recording) packed
 * [speakers[r]][clusters[cut][r]] at out_offsets; status int32 [cuts][b]: 0 counted; 1 not counted, the cut has more than 256 clusters
 * (the histogram is 32 x 256 counters in LDS); -1 not counted, clusters < 1 or entries that lead outside the buffers of the call (offsets,
 * speakers, a window or a label out of range).  A block that is not counted has totals 0 and writes no overlap.
 * Every output is an integer and integer adds commute (the histogram takes LDS atomic adds): the result is exact, independent of the
 * order of summation, and the same bytes every time.
 * Refused by name: b <= 0, cuts outside 1 .. 65535, negative totals, a missing array.  The device arrays are NOT checked on the host side
 * of this call (ops.diar_frames and ops.diar_confusion check the host arrays before the upload). */
int xv_diar_confusion(void* stream, const uint32_t* ref_mask, const uint8_t* scored, const int32_t* frame_window, const int64_t* frame_offsets,
                      const int64_t* win_offsets, const int32_t* speakers, int b, int64_t total_frames, int64_t total_n, const int32_t* labels,
                      const int32_t* clusters, const int64_t* out_offsets, int cuts, int64_t overlap_ints, int64_t* totals, int32_t* overlap,
                      int32_t* status);

/* VB-HMM clustering of x-vectors (VBx, Landini et al.: a Bayesian HMM whose states are speakers and whose state distributions come from
 * the PLDA model, started from the clusterer's labels), as recalled from BUT's VB_diarization.py and restated - agreement with a run of
 * that code is not pinned.  b recordings per call, one workgroup each, every iteration in the one launch, no hand-over between
 * workgroups: a recording's result depends on its own inputs only and is the same bits every time.
 * Inputs, all on the device: x, a packed fp32 buffer of x_floats floats; recording r's rows [t[r]][ld[r]], ld[r] >= d, start at float
 * x_offsets[r] (int64): vectors in the PLDA space in which the within-class covariance is I and the between-class covariance diag(phi)
 * (the affine step of the back end WITHOUT backend_plda_normalize); phi [d]; gamma_in, the initial responsibilities, recording r's
 * [t[r]][s[r]] (rows summing to 1) at the exclusive prefix of t * s; pi_in, the initial speaker priors, recording r's [s[r]] at the exclusive
 * prefix of s.  None of them is modified.
 * The arithmetic is part of the operation (tests/vbx_ref.py restates it: the definition in the log domain and the form computed).  Per
 * recording, rho = x * sqrt(phi), G_t = -(sum_d x_td^2 + d ln 2 pi) / 2, and an iteration is
 *   N_s = sum_t gamma_ts,  invL_sd = 1 / (1 + (fa / fb) N_s phi_d),  alpha_sd = (fa / fb) invL_sd sum_t gamma_ts rho_td
 *   logp_ts = fa (sum_d rho_td alpha_sd - sum_d (invL_sd + alpha_sd^2) phi_d / 2 + G_t)
 *   forward-backward over the HMM with initial distribution pi, transitions tr_ij = loop_prob [i = j] + (1 - loop_prob) pi_j and state
 *   likelihoods exp(logp): the new gamma and tll = log p(x)
 *   ELBO = tll + fb / 2 sum_sd (ln invL_sd - invL_sd - alpha_sd^2 + 1)
 *   pi_j <- gamma_0j + (1 - loop_prob) pi_j sum_{t >= 1} [sum_i A_{t-1,i}] p_tj B_tj / p(x) (A, B the forward and backward variables), then
 *   pi <- pi / sum pi
 *   stop after this iteration if it is not the first and ELBO - ELBO of the one before < epsilon (epsilon = -inf: never).
 * The speaker models and the scores are computed in double from the fp32 inputs, the recursions in fp32 in a per-frame scaled form: fa G_t, common to the speakers of a frame, leaves the scores and enters tll only;
 * b_tj = exp(logp'_tj - m_t), m_t the largest logp' of the frame among the speakers with pi > 0 (a speaker with pi = 0 has b = 0: it has
 * gamma 0 everywhere, stays at pi = 0 and makes no NaN); a_tj = b_tj (loop_prob a^_{t-1,j} + (1 - loop_prob) pi_j) (t = 0: b_0j pi_j),
 * n_t = sum_j a_tj, a^_t = a_t / n_t; w = b_{t+1} * B^_{t+1}, B^_t = (loop_prob w + (1 - loop_prob) sum_j pi_j w_j) / n_{t+1}, B^_{T-1} = 1;
 * gamma = a^ * B^; pi_j <- gamma_0j + (1 - loop_prob) pi_j sum_{t >= 1} b_tj B^_tj / n_t.  tll = sum_t (ln n_t + m_t) + fa sum_t G_t and the
 * ELBO's second term are accumulated in double; every sum runs in a fixed order.  The state between two iterations is (gamma, pi) in fp32
 * and nothing else: k iterations in one call are the same bits as k calls of one iteration.  With t = 1 there is no transition.
 * Outputs: gamma and pi (laid out as gamma_in and pi_in); elbo, double [b][max_iters], of which recording r's first n_iters[r] entries are
 * written; n_iters int32 [b], the iterations run; labels int32 [total_t], recording r's at the exclusive prefix of t: labels[t] = the
 * speaker with the largest gamma, the lowest on a tie.
 * total_t = sum t, total_ts = sum t * s, total_s = sum s, max_t, max_s: host values the caller states.  ws: xv_vbx_workspace_bytes bytes,
 * 16-byte aligned (per recording the scores in double, the partial sums of the models, b, a^, n and m).  Refused by name:
 * b <= 0, max_t outside 1 .. 2048 (the clusterer's cap), max_s outside 1 .. 32, d outside 1 .. 256, max_iters outside 1 .. 64, loop_prob
 * outside (0, 1), fa or fb not positive, an epsilon that is NaN, totals that do not fit, a workspace too small.  The device arrays are NOT
 * checked on the host side of this call (ops.vbx checks the host arrays before the upload); a recording whose entries would take the
 * kernel outside the buffers of the call is skipped and gets n_iters = -1.  NaN inputs and a pi without a positive entry are undefined. */
size_t xv_vbx_workspace_bytes(int64_t total_t, int64_t total_ts, int64_t total_s, int d);
int xv_vbx(void* stream, const float* x, int64_t x_floats, const int64_t* x_offsets, const int32_t* t, const int32_t* ld, const int32_t* s,
           int b, int d, int max_t, int max_s, int64_t total_t, int64_t total_ts, int64_t total_s, const float* phi, const float* gamma_in,
           const float* pi_in, float loop_prob, float fa, float fb, int max_iters, double epsilon, float* gamma, float* pi, double* elbo,
           int32_t* n_iters, int32_t* labels, void* ws, size_t ws_bytes);

/* The per-recording PCA in front of dense PLDA scoring (Kaldi's ivector-plda-scoring-dense --target-energy: callhome_diarization/v2 scores
 * with --target-energy 0.9), as recalled from ivector-plda-scoring-dense.cc and restated - the energy rule among it; agreement with a run
 * of Kaldi is not pinned.  b recordings per call, one workgroup each, no hand-over between workgroups: a recording's result depends on its
 * own inputs only and is the same bits every time and in every slot of a batch.
 * Inputs, all on the device: x, a packed fp32 buffer of x_floats floats; recording r's rows [n[r]][ld[r]], ld[r] >= d, start at float
 * x_offsets[r] (int64): centred, LDA-transformed, unit-length vectors (what the recipe feeds the scoring, up to ivector-normalize-length's
 * factor sqrt(d)).  w, bt: double [d][d], the within- and between-class covariances of the PLDA model at the scale sqrt(d),
 * W = T^-1 T^-T and B = T^-1 diag(psi) T^-T, symmetric; mu: double [d], the model's mean.  None of them is modified.
 * The arithmetic is part of the operation (tests/pca_plda_ref.py restates it).  Per recording, everything in double from the fp32 rows,
 * every sum in a fixed order:
 *   m = (1 / n) sum x_i,  C = (1 / n) sum x_i x_i^T - m m^T = P diag(s) P^T, s descending, negative round-off floored at 0
 *   the kept dimension: dim = 1, e = 0; while (e / sum s <= target) { e += s[dim - 1]; dim++; }  p = min(dim, d): one more than the smallest
 *   k whose first k eigenvalues hold more than `target` of the energy (Kaldi's loop; Kaldi has no cap at d).  n = 1 or sum s = 0: p = 0,
 *   "score with the global model" (Kaldi's "PCA failed"), and only p and s are written
 *   Q = the first p rows of P^T;  W' = Q W Q^T,  B' = Q B Q^T,  mu' = Q mu
 *   L = chol(W'), T1 = L^-1;  T1 B' T1^T = U diag(psi) U^T, psi descending, floored at 0;  T' = U^T T1
 * Both eigenproblems are solved by a cyclic Jacobi method in a fixed parallel (round-robin) order that stops after the first sweep in which
 * no off-diagonal element exceeds 2^-60 of the matrix's Frobenius norm, at most 40 sweeps (csrc/xv_backend_pca.hip states it).  A p above
 * the rank of C takes a direction from C's null space: arbitrary, as in Kaldi, but the same bits every time.
 * Outputs, d4 = d rounded up to 4, each fp32 value rounded once from double: p int32 [b]; a [b][d4][d4], recording r's map
 * sqrt(d) T' Q in its first p rows and d columns, the rest zero (sqrt(d), not sqrt(p): the PCA sees Kaldi's rows of length sqrt(d));
 * offset [b][d4] = -T' mu'; psi [b][d4]; the one-utterance tables of the log-likelihood ratio coef [b][2][d4] = (psi / (psi + 1), 1 / v),
 * v = 1 + psi / (psi + 1), g [b][d4] = 1 / (psi + 1), k0 [b] = -0.5 sum ln v + 0.5 sum ln(psi + 1), all zero behind p: operands of
 * xv_affine_forward (k = 1), xv_backend_plda_normalize with d = p, and xv_backend_plda_dense.  Diagnostics in double: s [b][d] (of the
 * unit-length rows' covariance), psi64 [b][d] (p entries written); sweeps int32 [b][2], the sweeps of the two eigenproblems.
 * p[r] = -1: recording r's entries (n outside 1 .. 2048, ld < d, rows outside x) would take the kernel outside the buffers of the call, it
 * is skipped; -2: an eigenproblem reached the sweep cap; -3: W' is not positive definite.  A recording with p <= 0 has nothing but p (and, for
 * p = 0, s and sweeps) written.  ws: xv_backend_pca_plda_workspace_bytes bytes, 16-byte aligned (four matrices of (d rounded up to 2)^2
 * doubles per recording).  Refused by name: b <= 0, d outside 1 .. 256, max_n (the largest n, a host value the caller states) outside
 * 1 .. 2048 (the clusterer's cap), a target outside (0, 1], a workspace too small.  The device arrays are NOT checked on the host side of
 * this call (ops.backend_pca_plda checks the host arrays before the upload).  NaN inputs are undefined. */
size_t xv_backend_pca_plda_workspace_bytes(int b, int d);
int xv_backend_pca_plda(void* stream, const float* x, int64_t x_floats, const int64_t* x_offsets, const int32_t* n, const int32_t* ld, int b,
                        int d, int max_n, double target, const double* w, const double* bt, const double* mu, int32_t* p, float* a,
                        float* offset, float* psi, float* coef, float* g, float* k0, double* s, double* psi64, int32_t* sweeps, void* ws,
                        size_t ws_bytes);

/* Kernel-layout weights for xv_affine_forward: wt[o][j*c_pad + c] = kernel[j][c][o]
 * (TF layout [k][C][O] of tdnn/tdnnX_{conv,dense}/kernel, tdnn.py:39,57,75,96,115,147,166);
 * columns c in [C, c_pad) are zero. */
int xv_prep_weight_fwd(void* stream, const float* kernel, int k, int c, int o, float* wt, int c_pad);
/* Kernel-layout weights for xv_affine_dgrad: wf[c][(k-1-j)*O + o] = kernel[j][c][o]. */
int xv_prep_weight_dgrad(void* stream, const float* kernel, int k, int c, int o, float* wf);

/* z[(b,t)][o] = bias[o] + sum_{j<k} sum_c x[b][t+j][c] * kernel[j][c][o]
 *   == tf.layers.conv2d(.., (1,k)) VALID, tdnn.py:39-44,57-62,75-80 and tf.layers.dense,
 *   tdnn.py:96-100,115-119,147-151,166-170 (k = 1, segs = rows, t_in = 1).
 * x: [segs][t_in][c_pad] spliced view, wt from xv_prep_weight_fwd, z: [segs*(t_in-k+1)][ldz].
 * If bn_part != NULL it receives per-128-row-tile column statistics of z (sum and centred
 * sum of squares, min, max: layout [4][tiles_m][o]) for xv_bn_finalize - the batch statistics of
 * tf.layers.batch_normalization(training=True), tdnn.py:46.  `ws` is scratch
 * (xv_op_workspace_bytes) used when the launcher splits the reduction.
 * Every GEMM operand (x, wt, dz - in split precision: each fp16 plane) must span less than 4 GB: the kernels address operand rows as
 * 32-bit byte offsets from the operand's base (an error is returned otherwise: split the batch). */
int xv_affine_forward(void* stream, const float* x, int segs, int t_in, int c_pad, int k,
                      const float* wt, const float* bias, float* z, int o, int ldz,
                      float* bn_part, void* ws, size_t ws_bytes);

/* dx[(b,s)][c] = sum_j sum_o dz[b][s-j][o] * kernel[j][c][o]  (gradient of the above w.r.t. x).
 * dz_pad: [segs][t_out + 2(k-1)][o] with k-1 ZERO rows before and after each segment
 * (written by xv_bn_backward_apply); wf from xv_prep_weight_dgrad ([c][k*o]); dx: [segs*(t_out+k-1)][c]. */
int xv_affine_dgrad(void* stream, const float* dz_pad, int segs, int t_out, int o, int k,
                    const float* wf, float* dx, int c, void* ws, size_t ws_bytes);

/* dkernel[j][c][o] = sum_{b,t} x[b][t+j][c] * dz[b][t][o]  (+ l2_scale * kernel[j][c][o],
 *   the gradient of tf.contrib.layers.l2_regularizer, tdnn.py:43 / trainer.py:357-358).
 * x: spliced view [segs][t_in][c_pad]; dz rows live in a buffer with `dz_seg_pitch` rows per
 * segment starting at row `dz_row0` (so the padded dz of xv_affine_dgrad can be used directly).
 * Output in TF layout [k][c][o] (padded channels dropped). */
int xv_affine_wgrad(void* stream, const float* x, int segs, int t_in, int c_pad, int k, int c,
                    const float* dz, int dz_seg_pitch, int dz_row0, int o,
                    const float* kernel, float l2_scale, float* dkernel,
                    void* ws, size_t ws_bytes);

/* out[n] = sum_r a[r][n]  (bias gradient, tf.layers bias_add grad). a: [rows][lda]. */
int xv_colsum(void* stream, const float* a, int rows, int n, int lda, float* out, void* ws, size_t ws_bytes);
/* Per-tile column statistics in the xv_affine_forward bn_part layout, for tensors that were
 * produced by a split reduction (segment-level layers). */
int xv_col_stats(void* stream, const float* z, int rows, int n, int ldz, float* bn_part);

/* tf.layers.batch_normalization(training=True) statistics, tdnn.py:46,64,82,102,121,153,177:
 * combine bn_part -> mean, biased var; scale = gamma*rsqrt(var+eps), shift = beta-mean*scale;
 * moving <- moving*momentum + batch*(1-momentum) (unbiased var if unbiased_moving != 0).
 * Outputs: mean[n], invstd[n], scale[n], shift[n]; optional zmin[n]/zmax[n] (range of z per channel) and
 * *amax |= max over the tensor of relu?(z*scale+shift) as float bits (atomicMax; zero it first) - the
 * exact output range the split-precision path scales its fp16 operand planes with. */
int xv_bn_finalize(void* stream, const float* bn_part, int rows, int n,
                   const float* gamma, const float* beta, float eps, float momentum, int unbiased_moving,
                   float* moving_mean, float* moving_var,
                   float* mean, float* invstd, float* scale, float* shift,
                   float* zmin, float* zmax, uint32_t* amax, int relu);
/* Inference statistics (training=False): scale/shift from the moving averages. */
int xv_bn_inference_scale(void* stream, int n, const float* gamma, const float* beta,
                          const float* moving_mean, const float* moving_var, float eps,
                          float* scale, float* shift);
/* a = relu?(z*scale + shift)   (tdnn.py:46-52: BN then tf.nn.relu). relu != 0 applies ReLU. */
int xv_bn_apply(void* stream, const float* z, int rows, int n, int ldz, const float* scale, const float* shift,
                int relu, float* a, int lda);
/* Backward of ReLU(BN(z)) given da (both dense [segs*t][n]): dy = da * (y>0); dgamma = sum dy*xhat; dbeta = sum dy;
 * dz = gamma*invstd*(dy - dbeta/rows - xhat*dgamma/rows) written into a segment-padded buffer
 * dz_pad [segs][t + 2*pad][n] (pad rows zeroed).  relu != 0 means a ReLU follows the BN.
 * dbias (optional): gradient of a bias added in FRONT of this BN = column sum of dz.  It is 0 in exact
 * arithmetic (BN removes the mean); TF's reduce_sum(dz) leaves rounding noise there, and so does this
 * (gamma*invstd*(sum dy - rows*mean dy)) without a separate pass over dz. */
int xv_bn_relu_backward(void* stream, const float* da, const float* z, int segs, int t, int n,
                        const float* gamma, const float* mean, const float* invstd,
                        const float* scale, const float* shift, int relu, int pad,
                        float* dz_pad, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes);
/* prelu, common.py:27-42: y[r][c] = relu(x) + alpha[c] * (x - |x|) / 2 = x > 0 ? x : alpha[c] * x  (tf.nn.leaky_relu: alpha = 0.2 everywhere).
 * Inside the engine the same non-linearity follows every BatchNorm when xv_config.relu_type says so. */
int xv_prelu_forward(void* stream, const float* x, int rows, int n, const float* alpha, float* y);
/* The activation that follows a BatchNorm in every op-level entry point that takes a `relu` flag (xv_bn_apply, xv_bn_apply_split,
 * xv_bn_relu_backward[_split|_pooled*], xv_stat_pool_forward_bn*, xv_segment_affine_bn_forward, xv_segment_dgrad_bn_backward,
 * xv_att_pool_backward_weights): network_relu_type of tdnn.py:24-30.
 *   slope == NULL (the default): tf.nn.relu.
 *   slope != NULL: y > 0 ? y : slope[c] * y with one device float per channel - prelu (common.py:27-42, slope = the layer's
 *     <layer>_relu/alpha variable; dalpha, if not NULL, receives d alpha[c] = sum over rows of da * min(y, 0) from the backward
 *     entry points) or lrelu (a constant 0.2 vector, dalpha = NULL).
 * The setting belongs to the CALLING THREAD and stays until the next call; set it around the calls of one layer and reset it with
 * (NULL, NULL).  The engine does exactly that per layer, so engine-level calls ignore and clear whatever was set here. */
int xv_set_activation(const float* slope, float* dalpha);
/* Backward of a bare ReLU (no BN in front): dz = da * (a > 0). */
int xv_relu_backward(void* stream, const float* da, const float* a, size_t count, float* dz);

/* ---------------------------------------------------------------------------------
 * Split precision ("f16x3"): the big TDNN contractions on the 16-bit matrix cores at fp32-class accuracy.
 * An fp32 tensor is carried as two fp16 planes [2][rows][ld] (ld multiple of 8, zero padded):
 * x*s = hi + lo with a power-of-two scale s derived from the tensor's max |x|, which travels in device
 * memory as the uint32 bits of a float (`amax`; producers atomicMax into it, so zero it first).  Products
 * hi.hi + hi.lo + lo.hi are accumulated in fp32 and multiplied by 1/(sA*sB) (2^-22 relative per product).
 * Same reference call sites as the fp32 entry points they mirror.
 * --------------------------------------------------------------------------------- */
int xv_amax(void* stream, const float* x, size_t count, uint32_t* amax_accum);
int xv_split_planes(void* stream, const float* src, int rows, int c, int lds, void* planes, int ldp, size_t plane_stride,
                    const uint32_t* amax);
/* planes <- relu?(z*scale+shift): BN(+ReLU) output written directly as the next layer's operand (tdnn.py:46-52) */
int xv_bn_apply_split(void* stream, const float* z, int rows, int n, int ldz, const float* scale, const float* shift, int relu,
                      const uint32_t* amax, void* planes, int ldp, size_t plane_stride);
/* Range of z (per channel) and of relu?(z*scale+shift) (whole tensor, into *amax) from the bn_part min/max planes,
 * for scale/shift that did not come from xv_bn_finalize (training=False: moving statistics). */
int xv_bn_output_range(void* stream, const float* bn_part, int rows, int n, const float* scale, const float* shift, int relu,
                       float* zmin, float* zmax, uint32_t* amax);
/* xv_bn_relu_backward with dz written as planes in the segment-padded layout; *dz_amax receives an upper bound of
 * max |dz| computed from per-channel max |dy| and the forward range zmin/zmax (xv_bn_finalize). */
int xv_bn_relu_backward_split(void* stream, const float* da, const float* z, int segs, int t, int n, const float* gamma,
                              const float* mean, const float* invstd, const float* scale, const float* shift,
                              const float* zmin, const float* zmax, int relu, int pad, void* dz_planes, int ldp,
                              size_t plane_stride, uint32_t* dz_amax, float* dgamma, float* dbeta, float* dbias, void* ws,
                              size_t ws_bytes);

/* xv_bn_relu_backward / _split for the layer whose output feeds statistics pooling (tdnn5): the upstream gradient is not
 * read from memory but evaluated from the pooled statistics pool_out [b][mean | std] (xv_stat_pool_forward_bn) and their
 * gradient dpool [b][2n] -  d a = dmean/t + dstd/(t*std) * (a - mean), a = relu?(z*scale + shift), zero where the
 * variance was clamped (pooling.py:28-29) - i.e. pooling backward + ReLU backward + BN backward in one pass over z.
 * rows = b*t, no segment padding. */
int xv_bn_relu_backward_pooled(void* stream, const float* pool_out, const float* dpool,
                               const float* weights /* [b*t] attention weights or NULL: d a = w*(dmean + dstd/std*(a - mean)) */, int b, int t,
                               const float* z, int n,
                               const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                               int relu, float* dz, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes);
/* The same pair with the pooling forward's by-product wpos [b][c] (the share of each chunk's frame weights on frames whose ReLU is
 * on; amax [b][c], optional: each chunk's largest activation): given wpos, the BatchNorm backward gets sum(dy) and sum(dy*xhat) in
 * closed form from the pooled statistics - no reduction pass over z (plain ReLU or no activation).  Same results up to rounding. */
int xv_stat_pool_forward_bn_aux(void* stream, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                                const float* weights, float* out, float* wpos, float* amax);
int xv_bn_relu_backward_pooled_aux(void* stream, const float* pool_out, const float* dpool, const float* weights, const float* wpos,
                                   int b, int t, const float* z, int n, const float* gamma, const float* mean, const float* invstd,
                                   const float* scale, const float* shift, int relu, float* dz, float* dgamma, float* dbeta,
                                   float* dbias, void* ws, size_t ws_bytes);
int xv_bn_relu_backward_pooled_split(void* stream, const float* pool_out, const float* dpool, const float* weights, int b, int t,
                                     const float* z, int n,
                                     const float* gamma, const float* mean, const float* invstd, const float* scale,
                                     const float* shift, const float* zmin, const float* zmax, int relu, void* dz_planes, int ldp,
                                     size_t plane_stride, uint32_t* dz_amax, float* dgamma, float* dbeta, float* dbias, void* ws,
                                     size_t ws_bytes);

/* xv_affine_forward / _dgrad / _wgrad on planes.  c_ld / o_ld: plane row pitches (multiples of 8). */
int xv_affine_forward_f16x3(void* stream, const void* x_planes, size_t x_plane_stride, const uint32_t* x_amax, int segs, int t_in,
                            int c_ld, int k, const void* wt_planes, size_t wt_plane_stride, const uint32_t* wt_amax,
                            const float* bias, float* z, int o, int ldz, float* bn_part);
int xv_affine_dgrad_f16x3(void* stream, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax, int segs, int t_out,
                          int o_ld, int k, const void* wf_planes, size_t wf_plane_stride, const uint32_t* wf_amax, float* dx, int c);
/* The same with the BN-backward reductions of the layer that owns dx fused into the epilogue: dx is d(relu(bn(z_below)));
 * part [ceil(rows/128)][3][c] = per-tile sum dd | sum dd*xhat | max |dd| with dd = dx masked by the ReLU - what the first pass of
 * xv_bn_relu_backward_split would compute by re-reading dx and z_below.  Feed it to xv_bn_relu_backward_split_from_part. */
int xv_affine_dgrad_bnstats_f16x3(void* stream, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax, int segs, int t_out,
                                  int o_ld, int k, const void* wf_planes, size_t wf_plane_stride, const uint32_t* wf_amax, float* dx, int c,
                                  const float* z_below, const float* scale, const float* shift, const float* mean, const float* invstd,
                                  float* part);
int xv_bn_relu_backward_split_from_part(void* stream, const float* part, int chunks, const float* da, const float* z, int segs, int t, int n,
                                        const float* gamma, const float* mean, const float* invstd, const float* scale,
                                        const float* shift, const float* zmin, const float* zmax, int pad, void* dz_planes, int ldp,
                                        size_t plane_stride, uint32_t* dz_amax, float* dgamma, float* dbeta, float* dbias, void* ws,
                                        size_t ws_bytes);
int xv_affine_wgrad_f16x3(void* stream, const void* x_planes, size_t x_plane_stride, const uint32_t* x_amax, int segs, int t_in,
                          int c_ld, int k, int c, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax,
                          int dz_seg_pitch, int dz_row0, int o_ld, int o, const float* kernel, float l2_scale, float* dkernel,
                          void* ws, size_t ws_bytes);

/* statistics_pooling, pooling.py:9-34: out[b] = concat(mean_t x, sqrt(max-masked var_t x)). */
int xv_stat_pool_forward(void* stream, const float* x, int b, int t, int c, float* out);
int xv_stat_pool_backward(void* stream, const float* x, const float* out, const float* dout,
                          int b, int t, int c, float* dx);

/* Statistics pooling over relu?(z*scale + shift) evaluated on the fly (tdnn5's BN + ReLU, tdnn.py:124-131, fused into
 * pooling.py:9-34): out[b] = [mean_t | std_t] of the activation, which is never written to memory. */
int xv_stat_pool_forward_bn(void* stream, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                            const float* weights /* [b*t] frame weights summing to 1 per chunk (self-attention), or NULL = 1/t */,
                            float* out);


/* ---- auxiliary losses (model/loss.py:985-1036; shipped in nnet_conf/..._r0.01.json and ..._mhe0.01.json) ----
 * ring loss: lambda * mean((||x|| - r)^2), r a trainable scalar ("softmax_ringloss/r").  Adds the value to *loss_accum,
 * lambda*2*(||x||-r)/rows to dnorm_accum[row] (what xv_add_norm_grad turns into d x) and writes d r.
 * MHE: lambda / (mean_{b,n}(2 - 2 wn[:,y_b].wn[:,n]) + 1e-6) on the column-normalised weights wn [c][ldn]; xv_mhe_loss adds the value
 * and leaves [g | u[c] | v[c]] in coef (1 + 2c floats) and the label histogram in counts (n ints); xv_mhe_add_grad adds
 * g*(u + counts[n]*v) to the gradient w.r.t. wn (before xv_loss_weight_backward). */
int xv_ring_loss(void* stream, const float* x, int rows, int n, int ldx, const float* r, float lambda, float* loss_accum,
                 float* dnorm_accum, float* dr);
int xv_mhe_loss(void* stream, const float* wn, int c, int n, int ldn, const int32_t* labels, int rows, float lambda, float* loss_accum,
                float* coef, int32_t* counts);
int xv_mhe_add_grad(void* stream, float* dwn, int c, int n, int ldn, const float* coef, const int32_t* counts);

/* ---- self-attention pooling, the shipped single-head form (model/pooling.py:37-192; nnet_conf/..._tdnn4_att.json) ----
 * The key network's dense layers run on the frame-level GEMMs; these are the pieces around them.
 *   score[r]   = scale * sum_c act(zk[r][c]) * query[c]        act: 0 = identity, 1 = relu, 3 = tanh (att_key_network_type, pooling.py:84-96)
 *   weights    = softmax over the t frames of each chunk        (pooling.py:148)
 *   pooled     = xv_stat_pool_forward_bn(..., weights, ...)     (pooling.py:151-164)
 * backward: d weights from the pooled statistics (the value path enters tdnn5's BN backward through
 * xv_bn_relu_backward_pooled*'s `weights`), softmax backward, then through the score into the key layer output:
 *   dzk[r][c] = dscore[r]*scale*query[c]*act'(zk),  dquery[c] = sum_r dscore[r]*scale*act(zk[r][c]),  dbias[c] = sum_r dzk[r][c]. */
int xv_att_score(void* stream, const float* zk, int rows, int n, int ldz, int act, const float* query, float scale, float* score);
int xv_softmax_segments(void* stream, const float* score, int b, int t, float* weights);
int xv_softmax_segments_backward(void* stream, const float* weights, const float* dweights, int b, int t, float* dscore);
int xv_att_pool_backward_weights(void* stream, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                                 const float* pool_out, const float* dpool, float* dweights);
int xv_att_key_backward(void* stream, const float* zk, int rows, int n, int act, const float* query, float scale, const float* dscore,
                        float* dzk, float* dquery, float* dbias, void* ws, size_t ws_bytes);
/* y[i] = act(z[i]), act as in xv_att_score (0 identity, 1 relu, 3 tanh): the "<name>_relu" / "<name>_tanh" endpoints of
 * common.py:150-213 dense_relu / dense_tanh for callers of pooling.self_attention (pooling.py:84-96). */
int xv_key_activation(void* stream, const float* z, size_t count, int act, float* y);
/* y[i] += x[i]  (the two gradient paths into tdnn4_relu: through tdnn5 and through the attention key network) */
int xv_add_inplace(void* stream, float* y, const float* x, size_t count);

/* ---- GhostVLAD / NetVLAD pooling (model/pooling.py:195-277), fp32 ----
 * x [b*t][c] is the value tensor (the last frame layer's ReLU output), kg = k centres + ghost clusters <= 64, c a multiple of 4.
 * The assignment logits x W + bias (pooling.py:242-246) and W's two gradients run on the dense GEMMs (xv_affine_forward / _wgrad /
 * _dgrad); these are the pieces around them.  No atomics: a call gives the same bits every time.
 *   a[r][j]   = softmax_j(logits[r][j]), j < kg; logits rows are ld >= kg floats apart (GEMM padding is never read)      pooling.py:249
 *   r[b][k]   = sum_t a[t][k] (x_t - centers[k]), n[b][k] = sum_t a[t][k], k < k centres (the ghosts are dropped)       pooling.py:258-266
 *               frames (optional, device [b]) / shrink: chunk i pools its first frames[i] - shrink rows only (batched extraction)
 *   out[b]    = [r_k rsqrt(max(|r_k|^2, 1e-12))]_k, and with final_norm the k*c row normalised once more the same way   pooling.py:268-271 */
int xv_vlad_softmax(void* stream, const float* logits, int rows, int kg, int ld, float* a);
/* dst[r][j] = j < cols ? src[r][j] : 0 for j < ldd (rows lds / ldd floats apart): the [c][kg] kernel of pooling.py:242-246 as a GEMM operand on
 * whole column quads (ldd = kg rounded up to 4, zero padding), and its gradient back (ldd = cols = kg < lds). */
int xv_vlad_repitch(void* stream, const float* src, int rows, int cols, int lds, float* dst, int ldd);
int xv_vlad_pool_forward(void* stream, const float* x, const float* a, const float* centers, int b, int t, int c, int k, int kg,
                         const int32_t* frames, int shrink, float* r, float* n);
int xv_vlad_normalize_forward(void* stream, const float* r, int b, int k, int c, int final_norm, float* out);
/* Backward of the above (what tf.gradients derives from pooling.py:249-271).
 *   dr from dout through both normalisations (a clamped norm passes the gradient through the constant 1e6: a zero residual stays finite)
 *   da[r][k] = (x_r - centers[k]) . dr[b][k] for k < k centres, 0 for the ghosts;  dx[r] = sum_k a[r][k] dr[b][k]  (one pass over x)
 *   dl[r][j] = a (da - sum_j a da), columns kg .. ld zeroed (ld <= 64)
 *   dc[k]    = -sum_b n[b][k] dr[b][k] for k < k centres, 0 for the ghosts, + l2 * centers[k] (pooling.py:256 regulariser), [kg][c] */
int xv_vlad_normalize_backward(void* stream, const float* r, const float* dout, int b, int k, int c, int final_norm, float* dr);
int xv_vlad_pool_backward(void* stream, const float* x, const float* a, const float* centers, const float* dr, int b, int t, int c, int k,
                          int kg, float* da, float* dx);
int xv_vlad_softmax_backward(void* stream, const float* a, const float* da, int rows, int kg, int ld, float* dl);
int xv_vlad_centers_backward(void* stream, const float* n, const float* dr, const float* centers, int b, int k, int kg, int c, float l2,
                             float* dc);

/* l2_scaling, common.py:45-58 (feature_norm:true, trainer.py:183-186). */
int xv_l2_scaling_forward(void* stream, const float* x, int rows, int n, float factor, float* y);
int xv_l2_scaling_backward(void* stream, const float* x, const float* dy, int rows, int n, float factor, float* dx);

/* Loss family, loss.py:9-355. */
enum { XV_LOSS_SOFTMAX = 0, XV_LOSS_ASOFTMAX = 1, XV_LOSS_AMSOFTMAX = 2, XV_LOSS_ARCSOFTMAX = 3,
       /* pairwise heads (below, "Pairwise loss heads"): no softmax/output variables whatever num_speakers says; options through xv_engine_set_pair_loss */
       XV_LOSS_SEMIHARD_TRIPLET = 4, XV_LOSS_ANGULAR_TRIPLET = 5,
       /* the GE2E training loss (below, "GE2E training loss"): no softmax/output variables either, two trainable scalars ge2e/w and ge2e/b;
        * options through xv_engine_set_ge2e_loss */
       XV_LOSS_GE2E = 6 };
/* ---- segment-level layers in one launch (rows <= XV_SEGMENT_MAX_ROWS chunks of a batch) ------------------------------
 * tf.layers.dense at tdnn.py:147,166 and the logits / gradient products of loss.py with M = chunks rows: the GEMM, its split-K sum
 * and the consumer's per-column work run in one launch.  ws: slabs (xv_op_workspace_bytes); tickets: one ZEROED uint32 per 32
 * output columns, left zeroed.  Optional row term (the ||x|| gradient of loss.py:122,147, what xv_add_norm_grad adds):
 * acc[m][:] += (row_norm[m] > 0 ? row_coef[m] / row_norm[m] : 0) * xrow[m][:]. */
#define XV_SEGMENT_MAX_ROWS 128
/* c[m][n] = sum_k a[m][k] * bt[n][k] + bias[n] (+ row term) */
int xv_segment_gemm(void* stream, const float* a, long lda, const float* bt, long ldb, int m, int n, int k, const float* bias,
                    const float* row_coef, const float* row_norm, const float* xrow, long ldx, float* c, long ldc,
                    void* ws, size_t ws_bytes, uint32_t* tickets);
/* dense + training-mode tf.layers.batch_normalization (+ activation) of tdnn.py:147-189: z = x . wt^T + bias, batch statistics over
 * the m rows (biased two-pass variance), moving averages, scale/shift, a = act(z*scale + shift) (a may be NULL).  Same arithmetic
 * as xv_affine_forward + xv_bn_finalize + xv_bn_apply (relu != 0: ReLU). */
int xv_segment_affine_bn_forward(void* stream, const float* x, long ldx, const float* wt, long ldw, int m, int n, int k,
                                 const float* bias, const float* gamma, const float* beta, float eps, float momentum,
                                 int unbiased_moving, float* moving_mean, float* moving_var, float* z, float* mean, float* invstd,
                                 float* scale, float* shift, int relu, float* a, void* ws, size_t ws_bytes, uint32_t* tickets);
/* d a = dy . wt^T (+ row term), then the backward of the BatchNorm (+ activation) layer whose pre-BN tensor is z [m][n]:
 * dz, dgamma, dbeta, dbias (xv_bn_relu_backward's arithmetic on m rows). */
int xv_segment_dgrad_bn_backward(void* stream, const float* dy, long lddy, const float* wt, long ldw, int m, int n, int k,
                                 const float* row_coef, const float* row_norm, const float* xrow, long ldx, const float* z,
                                 const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                                 int relu, float* dz, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes,
                                 uint32_t* tickets);

/* tf.nn.l2_normalize(w, dim=0), loss.py:104: inv_norm[n], wn[c][ldn] = w*inv, wnt[n][c] = wn^T.
 * normalize == 0 copies unnormalised (plain softmax, loss.py:30).  inv_norm carries the column's liveness: a column whose fp32
 * ss = sum_c w[c][n]^2 is below 1e-12f (clamped by the maximum()) holds exactly 1e6f = rsqrt(1e-12f); a live one holds
 * min(rsqrt(ss), 999999.9375f), one ulp below, and xv_loss_weight_backward keeps the projection term for it. */
int xv_loss_prep_weight(void* stream, const float* w, int c, int n, int normalize,
                        float* inv_norm, float* wn, int ldn, float* wnt);
/* Given logits = x . wn (+bias) [rows][ldl]: margin transform of the target logit, lambda
 * blend (fa = 1/(1+lambda)), mean sparse softmax cross entropy, and the gradients
 * dlogits [rows][ldl] (pad columns zeroed) and dnorm[rows] (= dL/d||x||, 0 for softmax).
 * loss_out: one float (mean over rows).  asoftmax: m in {1,2,4}. */
int xv_margin_softmax_rows(void* stream, int kind, const float* logits, int rows, int n, int ldl,
                           const float* x, int c, const int32_t* labels, float m, float lambda,
                           float* dlogits, float* dnorm, float* row_loss, float* loss_out);
/* dx[r][:] += dnorm[r] * x[r][:] / ||x[r]||  (the ||x|| paths of loss.py:122,147). */
int xv_add_norm_grad(void* stream, const float* x, const float* dnorm, int rows, int c, float* dx);
/* Gradient through l2_normalize: dw = inv*(dwn - live*wn*colsum(dwn*wn)) + l2_scale*w, live = inv_norm[n] != 1e6f (see xv_loss_prep_weight). */
int xv_loss_weight_backward(void* stream, const float* dwn, int lddwn, const float* wn, int ldn,
                            const float* inv_norm, const float* w, int c, int n, int normalize,
                            float l2_scale, float* dw, void* ws, size_t ws_bytes);

/* ---- Pairwise loss heads (loss.py:358-705), fp32: semi-hard triplet, angular triplet, end-to-end validation ----
 * x [b][d] is the embedding at row pitch ldx; b <= 1024 rows, d a multiple of 4, rows 16-byte aligned.  With G = x x^T:
 *   cosine     S_ij = clip(G_ij r_i r_j, -1, 1), r_i = rsqrt(max(G_ii, 1e-12))                                    common.py:97-110
 *   Euclidean  D2_ij = max((G_ii - 2 G_ij) + G_jj, 0) (exactly 0 on the diagonal); squared: d = D2, else d = sqrt(D2), 0 where D2 == 0  common.py:61-94
 *   semi-hard  sum over ordered pairs (x, i), equal labels, x != i, of max(margin + (d_xi - neg(x, i)), 0) / max(#pairs, 1e-16);
 *              neg = min{d_xy: other label, d_xy > d_xi}, else max{d_xy: other label}, else (one speaker) the row minimum
 *   angular    f = the positive side's transform by margin_kind / margin (loss.py:537-560); the negative side is S itself
 *              all:  sum over valid (a, p, n) of max(S_an - f(S_ap), 0) / (#{terms > 1e-12} + 1e-16)
 *              hard: mean over a of max(hn_a - hp_a, 0) with the fillers of loss.py:617-625
 * stats [4]: {pairs | valid triplets | anchors, 0 | positive triplets | anchors with a positive hinge, the fraction positive / valid (0 for
 * semi-hard), 0}.  Backward: maximum(x, 0) passes at x >= 0, the clip passes at its bounds, the masked sqrt entries get 0; a tie in a
 * min / max gives the whole gradient to the lowest index; the arc margin's 1 - S^2 is clamped at 1e-12 in the derivative (finite at |S| = 1).
 * No atomics: two calls give the same bits.  xv_pair_loss_forward leaves G, the gradient with respect to the pair matrix and
 * 1 / normaliser in ws; xv_pair_loss_backward (same cfg, x, b, d, ws) reads them and writes dx [b][d] at row pitch lddx (a multiple of 4). */
enum { XV_PAIR_SEMIHARD = 0, XV_PAIR_ANGULAR = 1 };
enum { XV_TRIPLET_ALL = 0, XV_TRIPLET_HARD = 1 };
typedef struct xv_pair_loss_config {
    int32_t struct_bytes;             /* = sizeof(xv_pair_loss_config) of the header the host was built against; anything else is refused */
    int32_t kind;                     /* XV_PAIR_* */
    int32_t squared;                  /* semi-hard: triplet_loss_squared */
    int32_t triplet_type;             /* angular: XV_TRIPLET_* */
    int32_t margin_kind;              /* angular: XV_LOSS_ASOFTMAX (margin 1, 2, 4) / _AMSOFTMAX / _ARCSOFTMAX */
    float margin;
    int32_t valid_speakers;           /* num_valid_speakers_per_batch / num_valid_segments_per_speaker: the N x M layout of a validation batch - read by */
    int32_t valid_segments;           /* the engine (xv_engine_loss_forward with with_margin = 0 on the angular kind), not by the op entry points below */
} xv_pair_loss_config;
size_t xv_pair_loss_workspace_bytes(int b, int d);      /* 0 (and xv_last_error) for a b or d outside the limits */
int xv_pair_loss_forward(void* stream, const xv_pair_loss_config* cfg, const float* x, int b, int d, int ldx, const int32_t* labels,
                         float* loss, float* stats, void* ws, size_t ws_bytes);
int xv_pair_loss_backward(void* stream, const xv_pair_loss_config* cfg, const float* x, int b, int d, int ldx, const int32_t* labels,
                          void* ws, size_t ws_bytes, float* dx, int lddx);
/* e2e_valid_loss (loss.py:637-705): x holds speakers x segments rows, speaker-major.  Rows l2-normalised, per-speaker centres (normalised
 * means), for a row's own speaker the normalised sum of the OTHER rows of that speaker, similarities x 20, mean sparse softmax cross-entropy. */
int xv_e2e_valid_loss(void* stream, const float* x, int speakers, int segments, int d, int ldx, float* loss, void* ws, size_t ws_bytes);

/* ---- GE2E training loss (loss.py:903-982; the NumPy statement model/test_utils.py:21-86), fp32 ----
 * x [B][d] at row pitch ldx holds B = speakers x segments rows, speaker-major; the layout comes from cfg and labels are not read.
 * segments >= 2, B <= 1024, d a multiple of 4, rows 16-byte aligned.  With l2(v) = v * rsqrt(max(|v|^2, 1e-12)) (l2_scaling(v, 1)):
 *   x^_i = l2(x_i);   centre c^_k = l2(sum of speaker k's x^);   exclusive centre e^_i = l2(sum of the OTHER rows of i's speaker)
 *   c_ik = x^_i . c^_k for k != spk(i),   c_i,own = x^_i . e^_i;      S_ik = |w| c_ik + b      (w, b: one device float each)
 *   softmax       mean over rows of the sparse softmax cross-entropy of S_i against the row's own speaker
 *   contrastive   mean over rows of 1 - sigmoid(S_i,own) + max(0, max_{k != own} sigmoid(S_ik)); the 0 is the masked entry of
 *                 reduce_max((1 - mask) * sigmoid): it alone remains with one speaker and carries no gradient
 * The kernels evaluate this from u = X^ X^T: x^_i . (sum of k) = sum_{m in k} u_im, |sum of k|^2 = sum_{m, m' in k} u_mm', and for the own
 * speaker the same sums over the pairs that do not touch row i.
 * Backward, with P = d loss / d S:  d w = sign(w) sum P_ik c_ik (sign(0) = 0, as tf.abs has it),  d b = sum P_ik (evaluated as that sum in
 * both types; rounding noise around 0 in softmax),  d x through the centres and the row norms.  maximum(., 1e-12) passes no gradient to a
 * clamped norm and the numerator keeps its factor rsqrt(1e-12); the contrastive maximum is taken where S is largest and a tie gives the
 * whole gradient to the lowest index.  No atomics, every sum in a fixed order: two calls give the same bits.
 * stats [4] (may be NULL): {d w, d b, 0, 0}.  xv_ge2e_loss_forward leaves G = x x^T, P, c and the norms in ws;
 * xv_ge2e_loss_backward (same cfg, x, d, w, b, ws) reads them and writes dx [B][d] at row pitch lddx, dw [1] and db [1].
 * ws in floats, with bp and np = B and speakers rounded up to 4 (diagnostics and tests read the forward's entries here):
 *   G [B][bp] | d loss / d u [B][bp] | its symmetrised form [B][bp] | row partials [bp][4] | {1 / B, d w, d b, ...} [8] |
 *   n_k [np] | P [B][np] without the mean's 1 / B | c [B][np] | the exclusive norms [bp] */
enum { XV_GE2E_SOFTMAX = 0, XV_GE2E_CONTRASTIVE = 1 };
typedef struct xv_ge2e_config {
    int32_t struct_bytes;             /* = sizeof(xv_ge2e_config) of the header the host was built against; anything else is refused */
    int32_t loss_type;                /* XV_GE2E_*: ge2e_loss_type */
    int32_t speakers;                 /* num_speakers_per_batch */
    int32_t segments;                 /* num_segments_per_speaker (not 1) */
    int32_t valid_speakers;           /* num_valid_speakers_per_batch / num_valid_segments_per_speaker: the layout of a validation batch - read by the */
    int32_t valid_segments;           /* engine (xv_engine_loss_forward with with_margin = 0), not by the op entry points below */
} xv_ge2e_config;
size_t xv_ge2e_loss_workspace_bytes(int speakers, int segments, int d);      /* 0 (and xv_last_error) for a layout or d outside the limits */
int xv_ge2e_loss_forward(void* stream, const xv_ge2e_config* cfg, const float* x, int d, int ldx, const float* w, const float* b,
                         float* loss, float* stats, void* ws, size_t ws_bytes);
int xv_ge2e_loss_backward(void* stream, const xv_ge2e_config* cfg, const float* x, int d, int ldx, const float* w, const float* b,
                          void* ws, size_t ws_bytes, float* dx, int lddx, float* dw, float* db);

/* sum over a flat range of 0.5*scale*w^2 accumulated into *out (regularization_loss). */
int xv_l2_reg_loss(void* stream, const float* w, size_t count, float scale, float* out_accum);

/* Optimisers, trainer.py:332-346.  g is scaled by grad_scale first (1/world for DP). */
int xv_sgd_update(void* stream, float* p, const float* g, size_t count, float lr, float grad_scale);
int xv_momentum_update(void* stream, float* p, const float* g, float* acc, size_t count,
                       float lr, float momentum, int nesterov, float grad_scale);
int xv_adam_update(void* stream, float* p, const float* g, float* m, float* v, size_t count,
                   float lr, float beta1, float beta2, float eps, int t, float grad_scale);
/* sum of squares of a flat range accumulated into *out (for tf.clip_by_global_norm): per-block partials added in index order, so the same
 * input gives the same bits on every call (no float atomics); xv_l2_reg_loss likewise. */
int xv_sumsq(void* stream, const float* g, size_t count, float* out_accum);

/* ---------------------------------------------------------------------------------
 * Engine level: the whole tdnn + loss graph of Trainer.build / sess.run(train_op)
 * --------------------------------------------------------------------------------- */
typedef struct xv_engine xv_engine;

typedef struct xv_config {
    int32_t struct_bytes;             /* = sizeof(xv_config) of the header the host was built against; anything else is refused (but the
                                       * size this struct had before the vlad_* fields were added at its end: see there) */
    int32_t feat_dim;                 /* dim, train.py:71 */
    int32_t num_speakers;             /* train.py:74 (0 => no loss head, predict only) */
    int32_t num_nodes_pooling_layer;  /* tdnn.py:111-113, default 1500 */
    int32_t num_nodes_last_layer;     /* tdnn.py:162-164, default 512 */
    int32_t last_layer_no_bn;         /* tdnn.py:173-174 */
    int32_t last_layer_linear;        /* tdnn.py:183-184 */
    int32_t feature_norm;             /* trainer.py:183 */
    float feature_scaling_factor;
    int32_t loss_kind;                /* XV_LOSS_* (trainer.py:234-250) */
    float margin_m;                   /* asoftmax_m / amsoftmax_m / arcsoftmax_m */
    float lambda_min, lambda_base, lambda_gamma, lambda_power; /* loss.py:144-145 */
    float weight_l2_regularizer;      /* tdnn.py:43 */
    float output_weight_l2_regularizer; /* loss.py:26-28; < 0 => use weight_l2_regularizer */
    float batchnorm_momentum;         /* tdnn.py:47 */
    float bn_epsilon;                 /* [TF] 1e-3 */
    int32_t fused_bn_unbiased_moving_var; /* SURVEY N4 switch (layers 1-3) */
    int32_t optimizer;                /* 0 sgd, 1 momentum, 2 adam (trainer.py:332-346) */
    float momentum;
    int32_t use_nesterov;
    float clip_gradient_norm;         /* trainer.py:408-410; <= 0 => clip_gradient:false */
    int32_t max_batch;                /* capacity: chunks per step */
    int32_t max_frames;               /* capacity: frames per chunk */
    int32_t precision;                /* XV_PRECISION_*: how the tdnn1-5 contractions are evaluated */
    int32_t pooling;                  /* XV_POOL_*: pooling_type, tdnn.py:133-138 */
    int32_t att_key0_nodes;           /* att_key_num_nodes[0]: dense+bn+relu on tdnn4_relu (pooling.py:78-82) */
    int32_t att_key1_nodes;           /* att_key_num_nodes[1]: the key dimension (pooling.py:84-96) */
    int32_t att_key_type;             /* att_key_network_type of the last key layer: 0 affine, 1 + relu, 2 + bn + relu, 3 + tanh */
    int32_t att_use_scale;            /* att_use_scale: scores / sqrt(key dim) (pooling.py:144-145) */
    int32_t aux_ring;                 /* "ring_loss" in aux_loss_func (loss.py:1003-1017); adds the variable softmax_ringloss/r */
    float ring_loss_init;             /* initial r (set by the host initialiser; the engine does not read it) */
    float ring_loss_lambda;
    int32_t aux_mhe;                  /* "mhe_loss" in aux_loss_func (loss.py:1018-1033); margin losses only (normalised weights) */
    float mhe_lambda;
    /* Frame-layer table.  0 = the reference's five layers (tdnn.py:35-127: contexts 5/5/7/1/1, widths 512 x 4 + num_nodes_pooling_layer).
     * Otherwise 3..XV_MAX_FRAME_LAYERS layers of (context k >= 1 contiguous frames, output channels); context 1 = dense.  Variables
     * are named tdnn<i>_conv / tdnn<i>_dense / tdnn<i>_bn as in the reference; the two segment-level layers follow as tdnn<F+1>,
     * tdnn<F+2>.  Extended tables have NO reference counterpart (BASELINE configs[4]). */
    int32_t num_frame_layers;
    int32_t frame_context[12];
    int32_t frame_width[12];
    int32_t relu_type;                /* XV_RELU_*: network_relu_type, tdnn.py:24-30 (no shipped config sets it) */
    /* capacity in rows = chunks x frames of one forward; 0 = max_batch * max_frames.  Batched extraction sets it (with a large
     * max_frames): a batch is many short utterances or a few long ones, never max_batch chunks of max_frames frames */
    int32_t max_rows;
    /* ghost_vlad pooling (pooling.py:195-277).  Added behind the fields of ABI version 3: a host built against the shorter struct
     * (struct_bytes = the offset of vlad_num_centers) is still accepted and reads as "no VLAD". */
    int32_t vlad_num_centers;         /* K >= 1 */
    int32_t vlad_num_ghosts;          /* G >= 0, K + G <= 64 */
    int32_t vlad_final_l2_norm;       /* pooling.py:270-271 */
} xv_config;
#define XV_MAX_FRAME_LAYERS 12
/* the non-linearity behind every BatchNorm: relu | prelu = relu(x) + alpha (x - |x|) / 2 with a trainable per-channel alpha
 * "<prefix>_relu/alpha" initialised to 0.01 (common.py:27-42) | tf.nn.leaky_relu (alpha 0.2) */
#define XV_RELU_RELU 0
#define XV_RELU_PRELU 1
#define XV_RELU_LRELU 2
#define XV_POOL_STATISTICS 0
/* self_attention in the shipped single-head form (nnet_conf/..._tdnn4_att.json): key network on tdnn4_relu, value = tdnn5_relu,
 * one head, key not split, no value network, no penalty term, no post non-linearity */
#define XV_POOL_SELF_ATTENTION 1
/* ghost_vlad / NetVLAD: key = value = the last frame layer's ReLU output, no key / value networks; fp32 engine only.  The output is
 * vlad_num_centers * num_nodes_pooling_layer columns wide */
#define XV_POOL_GHOST_VLAD 2
/* fp32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32 products) */
#define XV_PRECISION_F32 0
/* split precision: three fp16 MFMA products of (hi,lo) pieces per fp32 product, fp32 accumulate (2^-22 relative) */
#define XV_PRECISION_F16X3 1

int xv_engine_create(const xv_config* cfg, xv_engine** out);
void xv_engine_destroy(xv_engine* e);

/* Variable table (TF names/shapes in graph order, e.g. "tdnn/tdnn1_conv/kernel" [1,5,D,512]). */
int xv_engine_num_variables(const xv_engine* e);
/* name: pointer to a static string; shape: up to 4 dims written, returns rank via *rank;
 * offset in floats into the variables buffer; trainable flag. */
int xv_engine_variable_info(const xv_engine* e, int index, const char** name, int32_t shape[4],
                            int32_t* rank, size_t* offset, int32_t* trainable);
/* Flat sizes in floats: all variables (trainable first, then BN moving statistics),
 * trainable only (= gradient buffer), optimiser state. */
size_t xv_engine_variables_count(const xv_engine* e);
size_t xv_engine_trainable_count(const xv_engine* e);
size_t xv_engine_optimizer_state_count(const xv_engine* e);
/* Caller-owned device buffers (e.g. torch tensors): variables, gradients, optimiser state. */
int xv_engine_bind(xv_engine* e, float* variables, float* grads, float* opt_state);

/* tdnn(features) (+ entire_network's l2_scaling).  features: [b][t][feat_dim].
 * training != 0: batch statistics + moving-average update (is_training=True). */
int xv_engine_forward(xv_engine* e, void* stream, const float* features, int b, int t, int training);
/* Inference forward (is_training=False, trainer.py:708-726) over a batch of utterances of DIFFERENT lengths, the batched form of the loop
 * extract.py:64-93 runs one utterance at a time: chunk i of features [b][t][feat_dim] holds frames[i] valid frames (receptive field <=
 * frames[i] <= t) followed by padding (finite values, e.g. zeros).  The frame layers are valid convolutions, so the first
 * frames[i] - (receptive field - 1) output frames of chunk i do not see the padding; pooling (and the attention softmax) use exactly
 * those.  Segment-level endpoints ("pooling", "tdnn6_dense", ...) are per chunk as usual; frame-level endpoints keep their padded rows.
 * frames: device array [b]. */
int xv_engine_forward_lengths(xv_engine* e, void* stream, const float* features, int b, int t, const int32_t* frames);
/* loss_network(features, labels) + gradients of loss + regulariser w.r.t. every trainable
 * variable into the bound gradient buffer.  global_step feeds the lambda schedule
 * (trainer.py:505-508).  stage: -1 = everything; 0..XV_BWD_STAGES-1 = that slice only (lets the
 * host overlap the gradient all-reduce of finished slices with the rest of the backward). */
#define XV_BWD_STAGES 4
int xv_engine_loss_forward(xv_engine* e, void* stream, const int32_t* labels, int global_step, int with_margin);
/* loss_kind XV_LOSS_SEMIHARD_TRIPLET / _ANGULAR_TRIPLET: the head's options (cfg->kind must match the engine's loss_kind), handed over after
 * create; xv_engine_loss_forward without them is refused by name.  With with_margin = 0 the angular kind evaluates xv_e2e_valid_loss on
 * valid_speakers x valid_segments rows (trainer.py:272-275; no backward follows it), the semi-hard kind the same loss as in training.
 * Stage 0 of the backward then has no head weight gradient: xv_pair_loss_backward writes d out, and tdnn7 / tdnn6 run unfused from there. */
int xv_engine_set_pair_loss(xv_engine* e, const xv_pair_loss_config* cfg);
/* loss_kind XV_LOSS_GE2E: the head's options, handed over after create; xv_engine_loss_forward without them is refused by name.  The head
 * declares the trainable scalars ge2e/w and ge2e/b (outside the L2 regulariser; clipped, updated, all-reduced and stored like any other
 * variable), no softmax/output variables, no auxiliary losses.  with_margin = 1: xv_ge2e_loss_forward on speakers x segments rows (a batch
 * of another size is refused); with_margin = 0: xv_e2e_valid_loss on valid_speakers x valid_segments rows (no backward follows it).
 * Stage 0 of the backward: xv_ge2e_loss_backward writes d out, d w and d b; tdnn7 / tdnn6 run unfused from there. */
int xv_engine_set_ge2e_loss(xv_engine* e, const xv_ge2e_config* cfg);
int xv_engine_backward(xv_engine* e, void* stream, int stage);
/* Staged backward without the join at the end of stages 0..2: `stream` does not wait for the engine's weight-gradient stream,
 * so the next stage's data-gradient chain keeps overlapping it.  The slice of stage k is complete on any stream that called
 * xv_engine_stage_wait(e, that_stream, k) - typically the communication stream the slice's all-reduce is enqueued on.  The last
 * stage joins on `stream` as xv_engine_backward does (xv_engine_apply may follow on `stream`); a different consumer stream
 * still has to call xv_engine_stage_wait for it. */
int xv_engine_backward_async(xv_engine* e, void* stream, int stage);
int xv_engine_stage_wait(xv_engine* e, void* waiter_stream, int stage);
/* Data parallelism for hosts without torch.distributed (the reference has no multi-GPU path: model/trainer.py:349 withholds its
 * tower design): sum-all-reduce, in place, of the gradient slice that backward stage `stage` completed - after
 * xv_engine_backward_async(e, compute_stream, stage) - over the RCCL communicator the host created (ncclComm_t passed as void*; one
 * rank per GPU), enqueued on `comm_stream` behind the stage's completion events, so the collective of stage k overlaps the backward
 * of stages k+1...  Call it for stages 0..XV_BWD_STAGES-1 in order (largest slice - the speaker matrix - first), then
 * xv_engine_allreduce_wait(e, compute_stream) and xv_engine_apply(..., grad_scale = 1 / world size, ...).  BatchNorm statistics stay
 * local to each rank.  RCCL is looked up in the process at first use (no link-time dependency). */
int xv_engine_allreduce(xv_engine* e, void* comm_stream, int stage, void* rccl_comm);
/* `stream` waits for every all-reduce enqueued so far through xv_engine_allreduce. */
int xv_engine_allreduce_wait(xv_engine* e, void* stream);
/* [begin,end) float range of the gradient buffer completed by backward stage `stage`. */
int xv_engine_stage_grad_range(const xv_engine* e, int stage, size_t* begin, size_t* end);
/* optimiser step on the bound buffers (after the gradient all-reduce). t = 1-based update count. */
int xv_engine_apply(xv_engine* e, void* stream, float lr, float grad_scale, int t);
/* bytes of device memory the engine's arena holds (activations, gradients' scratch, dz slots, workspaces) - diagnostics and tests */
size_t xv_engine_arena_bytes(const xv_engine* e);
/* scalars of the last step, device pointers to 1 float each: raw loss, regularisation loss */
int xv_engine_loss_ptrs(xv_engine* e, float** raw_loss, float** reg_loss);
/* Diagnostics: device pointer to 1 float, the sum of squares over the gradient buffer [0, trainable count) as the last xv_engine_apply
 * with clip_gradient_norm > 0 took it - before grad_scale: that update's global norm is sqrtf(*sumsq) * grad_scale.  Read-only. */
int xv_debug_engine_clip_sumsq(xv_engine* e, float** sumsq);
/* endpoint by reference name ("tdnn1_conv", ..., "pooling", "tdnn6_dense", "output", "logits"; ghost_vlad: "vlad_key", "vlad_weights",
 * "vlad_centers"):
 * device pointer, rows, cols, leading dimension of the most recent forward. */
int xv_engine_endpoint(xv_engine* e, const char* name, float** ptr, int32_t* rows, int32_t* cols, int32_t* ld);
/* 1 (default): weight gradients run on an internal second HIP stream beside the data-gradient chain;
 * 0: everything in order on the caller's stream (used to time kernels in isolation). */
int xv_engine_set_concurrency(xv_engine* e, int enabled);
/* Mark kernel-layout weight copies stale (call after writing the variables buffer directly). */
int xv_engine_invalidate_weights(xv_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* XVECTOR_HIP_H */
