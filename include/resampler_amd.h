/*
 * resampler_amd.h -- C ABI of the MI355X-native resampling engine (libresampler_amd.so).
 *
 * Drop-in boundary for the hot path of hasenbanck/resampler v0.5.1: each entry point names the
 * reference interface it replaces (file:line relative to the reference repository).  Plain
 * pointers and sizes only; all buffers are interleaved f32 frames, all counts are numbers of f32
 * values across all channels exactly as in the reference (src/resampler_fir.rs:617-620).
 *
 * Pointers named `in`/`out` are HOST pointers; pointers named `d_in`/`d_out` are DEVICE (HBM)
 * pointers on the handle's device.  `stream` is a hipStream_t passed as void*.  NULL = the handle's
 * (or batch's) OWN stream, created hipStreamNonBlocking: work enqueued there is NOT ordered against
 * the legacy default stream -- a caller whose buffers are produced / consumed on the default stream
 * passes RSMP_STREAM_LEGACY (== hipStreamLegacy) instead, or a stream of its own and orders that.
 * Device entry points are asynchronous on `stream`; the returned counts
 * are exact and available immediately (they come from the host-side mirror of the reference
 * state machine, not from the GPU).
 *
 * What a caller may do with its streams (tests/test_stream_order_gpu.py):
 *  - every device entry point: a call is ordered behind everything enqueued on `stream` before it, and work enqueued there
 *    after it sees its results -- however busy the stream is;
 *  - every entry point: change streams from one call of a handle / batch to the next (the library orders the calls of one
 *    handle across the change), and pass RSMP_STREAM_LEGACY;
 *  - every entry point: destroy a stream once the caller has synchronized it (a FIR handle's calls -- rsmp_fir_resample_device,
 *    _resample_bulk_device, rsmp_fir_seek, batch launches planned on the host -- and the FFT entry points order a change of
 *    streams through an event of the handle's last launch, never through the old stream; a lock-step batch synchronizes
 *    its last stream when the stream changes, and forgets the caller's streams in rsmp_fir_lockstep_sync, which the caller
 *    calls before destroying the stream a step or run was enqueued on; rsmp_fir_batch_resample_bulk_device(_ex) through the
 *    device planner returns when the launch is through);
 *  - FFT entry points only: destroy a stream right after the call, without synchronizing it (hipStreamDestroy lets the
 *    enqueued work finish).
 *
 * There is no CPU fallback: every compute entry point fails with RSMP_ERR_NO_DEVICE when no HIP
 * device is present.  The rsmp_*_plan_* / rsmp_design_* entry points are host-only (filter
 * design, FFT planning, and the (consumed, produced) state machine) and work without a GPU.
 */
#ifndef RESAMPLER_AMD_H
#define RESAMPLER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The legacy default stream as a `stream` argument (the value of hipStreamLegacy); NULL does not mean it. */
#define RSMP_STREAM_LEGACY ((void*)1)

/* ---- status codes: 1 and 2 are ResampleError (src/error.rs:3-8) ------------------------------- */
enum {
    RSMP_OK = 0,
    RSMP_ERR_INVALID_INPUT_BUFFER_SIZE = 1,  /* ResampleError::InvalidInputBufferSize  */
    RSMP_ERR_INVALID_OUTPUT_BUFFER_SIZE = 2, /* ResampleError::InvalidOutputBufferSize */
    RSMP_ERR_INVALID_ARGUMENT = 3,           /* where the reference panics (resampler_fir.rs:302-309) */
    RSMP_ERR_NO_DEVICE = 4,
    RSMP_ERR_HIP = 5,
    RSMP_ERR_CAPACITY = 6                    /* caller-provided array too small (bulk/plan calls) */
};

/* enum SampleRate (src/lib.rs:167-188), same order as the reference. */
enum {
    RSMP_HZ22050 = 0, RSMP_HZ16000, RSMP_HZ32000, RSMP_HZ44100, RSMP_HZ48000,
    RSMP_HZ88200, RSMP_HZ96000, RSMP_HZ176400, RSMP_HZ192000, RSMP_HZ384000
};
/* enum Latency (src/resampler_fir.rs:139-149): taps = 16, 32, 64, 128. */
enum { RSMP_LATENCY_SAMPLE8 = 0, RSMP_LATENCY_SAMPLE16, RSMP_LATENCY_SAMPLE32, RSMP_LATENCY_SAMPLE64 };
/* enum Attenuation (src/resampler_fir.rs:102-110): Kaiser beta = 7, 10, 13. */
enum { RSMP_ATTENUATION_DB60 = 0, RSMP_ATTENUATION_DB90, RSMP_ATTENUATION_DB120 };

/* FIR kernel selection (rsmp_fir_set_kernel).  AUTO picks PERIODIC when the rate pair reduces to
 * a small rational and the launch is long enough, GENERIC otherwise.  PERIODIC runs streams
 * on the matrix cores where the geometry allows: the split kernel (every f32 operand as the sum
 * of two fp16 values of the scaled operand, three fp16 MFMA products accumulated in f32; RSMP_FIR_SPLIT_PLANES=3
 * selects three bf16 planes / six products, exact in every bit) for rate pairs with
 * 16..160 classes such as 44.1 <-> 48 kHz and 1 .. 16 channels (channel pairs), the exact-f32 MFMA
 * kernel for other 2-channel geometries, the vector kernel otherwise.  PERIODIC_F32 keeps
 * every product in f32 (exact-f32 MFMA or vector kernels, never the split one); PERIODIC_VECTOR forces
 * the packed-FMA vector kernel for every channel count.  All produce the same results within the
 * 1e-6 RMS gate (measured against the CPU path: about 1.2e-7 RMS each).
 * Non-finite and out-of-range input: every kernel gives the reference's answer -- the same outputs are
 * finite, +inf, -inf or NaN (src/fir/avx.rs:25-58).  The PERIODIC kernels check the sums they store; a
 * launch that saw a non-finite sum (an inf / NaN sample, or in the split kernel a sample of magnitude
 * >= 16, beyond its fp16 planes) is followed by a repair launch that re-evaluates the affected 1024-frame
 * chunks in the reference's own two-row form (tests/test_fir_gpu.py::
 * test_non_finite_and_huge_input_match_the_reference).  One residue: at outputs whose exact position is a
 * multiple of 1/1024 frame the reference's inf-versus-NaN depends on the sign of an ~1e-12 rounding residue
 * of its f64 position; the repair pass may say NaN where the reference says inf or vice versa (GENERIC, which
 * replays the exact f64 positions, does not).  Clean audio never takes the repair path. */
enum { RSMP_FIR_KERNEL_AUTO = 0, RSMP_FIR_KERNEL_GENERIC = 1, RSMP_FIR_KERNEL_PERIODIC = 2,
       RSMP_FIR_KERNEL_PERIODIC_VECTOR = 3, RSMP_FIR_KERNEL_PERIODIC_F32 = 4 };
/* Dither of PCM output (no counterpart in the reference, which writes f32): none, or triangular noise of +-1 LSB added before
 * rounding -- the rule is stated at rsmp_f32_to_pcm_dither. */
enum { RSMP_DITHER_NONE = 0, RSMP_DITHER_TPDF = 1 };
/* Spectral shape of the TPDF noise (read only with RSMP_DITHER_TPDF): white -- the noise rsmp_f32_to_pcm_dither states --, or
 * high-pass: the difference of two consecutive values of ONE uniform sequence per channel, zero at DC and doubled at Nyquist --
 * the rule is stated at rsmp_f32_to_pcm_shaped.  No error feedback anywhere: the noise stays a function of the seed and the index. */
enum { RSMP_DITHER_SHAPE_WHITE = 0, RSMP_DITHER_SHAPE_HIGHPASS = 1 };

const char* rsmp_last_error(void);          /* thread-local message of the last failing call */
int rsmp_device_count(void);                /* number of HIP devices, 0 when there is none   */
const char* rsmp_version(void);
/* impl From<SampleRate> for u32 (src/lib.rs:219-236); 0 for an invalid enum value. */
uint32_t rsmp_sample_rate_hz(int sample_rate);

/* ============================ ResamplerFir (src/resampler_fir.rs) =============================== */
typedef struct rsmp_fir rsmp_fir;
/* What a PCM writer did to the values it was given (no counterpart in the reference, which writes f32; SoX prints "clipped N
 * samples").  32 bytes.  The rule is stated at rsmp_f32_to_pcm_stats.  Two sets merge field by field: the counts add, the peak
 * is the larger one. */
typedef struct rsmp_pcm_stats {
    uint64_t values;     /* values quantised */
    uint64_t clipped;    /* ... of which lay outside the code range and were saturated */
    uint64_t nans;       /* ... of which were NaN and were stored as 0 (not counted as clipped) */
    float peak;          /* largest |x| of the values that were not NaN, before scaling and dither; +inf possible; 0 if none.
                          * Under an output gain: of the gained values (rsmp_f32_to_pcm_gain).  What a second pass needs to choose its
                          * gain: rsmp_pcm_normalise_gain */
    uint32_t reserved;   /* 0 */
} rsmp_pcm_stats;

/* ResamplerFir::new (resampler_fir.rs:252-266).  NULL + rsmp_last_error() on failure. */
rsmp_fir* rsmp_fir_new(size_t channels, int input_rate, int output_rate, int latency,
                       int attenuation, int device);
/* ResamplerFir::new_from_hz (resampler_fir.rs:295-404); zero rates -> NULL (reference panics). */
rsmp_fir* rsmp_fir_new_from_hz(size_t channels, uint32_t input_rate_hz, uint32_t output_rate_hz,
                               int latency, int attenuation, int device);
/* Drop (resampler_fir.rs:61-67 et al.). */
void rsmp_fir_free(rsmp_fir* r);
/* ResamplerFir::buffer_size_output (resampler_fir.rs:456-465). */
size_t rsmp_fir_buffer_size_output(const rsmp_fir* r);
/* ResamplerFir::delay (resampler_fir.rs:630-632). */
size_t rsmp_fir_delay(const rsmp_fir* r);
/* ResamplerFir::reset (resampler_fir.rs:638-642). */
void rsmp_fir_reset(rsmp_fir* r);
/* fmt::Debug fields (resampler_fir.rs:203-211). */
size_t rsmp_fir_channels(const rsmp_fir* r);
size_t rsmp_fir_taps(const rsmp_fir* r);
size_t rsmp_fir_phases(const rsmp_fir* r);
/* The reference's private streaming state (resampler_fir.rs:189-192: read_position, available_frames,
 * position), for tests and checkpoints: it must equal the reference's after the same calls. */
void rsmp_fir_state(const rsmp_fir* r, size_t* read_position, size_t* available_frames, double* position);
int rsmp_fir_set_kernel(rsmp_fir* r, int kernel);
/* Measurement hook: when enabled, the convolution launch(es) of every call made through this
 * handle (the first handle of a batch call) are bracketed by HIP events on the launch stream;
 * rsmp_fir_last_kernel_ms waits for the last one and returns its duration. */
int rsmp_fir_set_profiling(rsmp_fir* r, int enable);
int rsmp_fir_last_kernel_ms(rsmp_fir* r, float* ms);
/* Mean over the (up to 64) most recent launches made since profiling was enabled; no host sync
 * happens between those launches, so this is the kernel's duration inside a timed region. */
int rsmp_fir_mean_kernel_ms(rsmp_fir* r, float* ms, size_t* launches);
/* Which kernel the handle's last launch used (diagnostic, for benchmark reports): 0 generic
 * (any ratio), 1 periodic vector kernel, 2 no longer returned (it was the periodic vector kernel with
 * double-buffered workgroups), 3 periodic exact-f32 matrix-core kernel, 4 periodic split matrix-core kernel with
 * three bf16 planes per operand (RSMP_FIR_SPLIT_PLANES=3), 5 periodic split matrix-core kernel with
 * two fp16 planes per operand (the default for rate pairs it has a geometry for); negative: invalid
 * handle. */
int rsmp_fir_kernel_variant(const rsmp_fir* r);

/* ResamplerFir::resample (resampler_fir.rs:509-621): one call, host buffers, synchronous. */
int rsmp_fir_resample(rsmp_fir* r, const float* in, size_t in_len, float* out, size_t out_len,
                      size_t* consumed, size_t* produced);
/* Same call with HBM-resident buffers, asynchronous on `stream`. */
int rsmp_fir_resample_device(rsmp_fir* r, const float* d_in, size_t in_len, float* d_out,
                             size_t out_len, size_t* consumed, size_t* produced, void* stream);

/* Bulk form: the result is DEFINED as what the reference driver loop resample_batch_fir
 * (resample/src/main.rs:226-254) returns when it feeds `chunk_len`-value slices (the CLI uses
 * 512) through resample() with a buffer_size_output() scratch: same output values, same total
 * count, same per-call (consumed, produced) pairs (written to calls[2*i], calls[2*i+1] for the
 * first max_calls calls; calls may be NULL).  One kernel launch for the whole buffer.
 * out_cap must hold every produced value (RSMP_ERR_CAPACITY otherwise; use
 * rsmp_fir_bulk_output_bound). */
size_t rsmp_fir_bulk_output_bound(const rsmp_fir* r, size_t in_len, size_t chunk_len);
int rsmp_fir_resample_bulk(rsmp_fir* r, const float* in, size_t in_len, size_t chunk_len,
                           float* out, size_t out_cap, size_t* consumed, size_t* produced,
                           size_t* calls, size_t max_calls, size_t* n_calls);
int rsmp_fir_resample_bulk_device(rsmp_fir* r, const float* d_in, size_t in_len, size_t chunk_len,
                                  float* d_out, size_t out_cap, size_t* consumed, size_t* produced,
                                  size_t* calls, size_t max_calls, size_t* n_calls, void* stream);

/* Batch form: n independent resampler instances (all on the same device), stream i processing
 * d_in[i] -> d_out[i] with bulk semantics, all in ONE launch per kernel flavour.  This is the
 * unit that is sharded across GPUs (one process per GPU, a contiguous range of streams each). */
int rsmp_fir_batch_resample_bulk_device(rsmp_fir* const* rs, size_t n, const float* const* d_in,
                                        const size_t* in_lens, size_t chunk_len,
                                        float* const* d_out, const size_t* out_caps,
                                        size_t* consumed, size_t* produced, void* stream);
/* The same with the PLANNER named.  A launch plans every distinct state among its streams on the host (streams in one state that are
 * fed the same amount share a plan): ~30 us of a core per state and thousand calls -- 2-3 ms for 64 streams x 4096 calls in 64 states
 * around a 0.3 ms kernel.  planner = 1 plans on the DEVICE instead (rsmp_fir_lockstep_run_bulk on a lock-step batch over the same
 * handles, which the library keeps from launch to launch for as long as the handles are touched through nothing else; the states are
 * written back into the handles before the call returns, so the call returns when the launch is THROUGH, not when it is enqueued);
 * planner = 0 never; planner = -1 -- what rsmp_fir_batch_resample_bulk_device does -- where the batch has at least 16 different
 * states.  The device planner takes batches of one channel count, whole calls (in_lens[i] a multiple of chunk_len) of at most 2048
 * frames, at least eight of them, and output buffers with room for the outputs the launch makes in exact arithmetic + 2 frames
 * (rsmp_fir_bulk_output_bound's value is always enough for a stream's first launch; it grows with the frames a stream has
 * buffered, so it is no test); anything else is planned on the host whatever `planner` says.  Buffer lengths: planner = -1 takes
 * batches of ONE buffer length only; planner = 1 also takes batches whose in_lens differ (zero among them: such a stream makes no
 * call; the eight calls are then asked of the longest stream) through rsmp_fir_lockstep_run_bulk_v -- unless a stream has so many
 * frames buffered that a call could accept less than it is offered (buffered + chunk frames > 4096), which goes to the host
 * planner before anything is launched.
 * *planned_on_device (may be null): which it was.  Same (consumed, produced), samples and end states either way. */
int rsmp_fir_batch_resample_bulk_device_ex(rsmp_fir* const* rs, size_t n, const float* const* d_in,
                                           const size_t* in_lens, size_t chunk_len,
                                           float* const* d_out, const size_t* out_caps,
                                           size_t* consumed, size_t* produced, void* stream, int planner, int* planned_on_device);
/* The same over a two-channel WAV file's samples as they are in the file (resample/src/main.rs:128-137): d_pcm[i] =
 * little-endian PCM of `bits` (16 / 24 / 32) per sample, in_lens[i] SAMPLES (2 per frame), 4-byte aligned.  The samples are
 * converted where the kernels read their input (`sample as f32 / (1 << (bits - 1)) as f32`, with the reference's 32-bit
 * divisor -2^31): the output equals rsmp_pcm_to_stereo_f32_device + rsmp_fir_batch_resample_bulk_device's within the
 * kernels' usual tolerance (the same samples reach the same arithmetic), and the launch reads 2 - 4 bytes a sample
 * instead of the conversion pass's PCM + 4 written + 4 read.  Long launches need the 128-tap rate pairs of the split
 * kernel (44.1 <-> 48 kHz, 96 -> 44.1 / 48 kHz ...: RSMP_ERR_INVALID_ARGUMENT otherwise -- convert first); at most one
 * launch's worth of input per stream (46 M outputs). */
int rsmp_fir_batch_resample_bulk_pcm_device(rsmp_fir* const* rs, size_t n, const void* const* d_pcm, int bits,
                                            const size_t* in_lens, size_t chunk_len, float* const* d_out,
                                            const size_t* out_caps, size_t* consumed, size_t* produced, void* stream);
/* The other half of a file-to-file pipeline: the output as a WAV file stores it.  d_out_pcm[i] receives little-endian PCM of
 * `out_bits` (16 / 24 / 32; 24-bit packed at 3 bytes a sample), 4-byte aligned, with room for out_caps[i] SAMPLES; every value
 * the f32 entry would have written is quantised where the kernels store it (the rule: rsmp_f32_to_pcm below), so the bytes are
 * exactly rsmp_f32_to_pcm_device's of rsmp_fir_batch_resample_bulk_device's output and the f32 never reaches HBM.  d_in[i] is
 * interleaved f32 (in_bits = 0) or PCM of in_bits (16 / 24 / 32) as in rsmp_fir_batch_resample_bulk_pcm_device; in_lens in
 * values / samples.  Counts, end states, the buffered frames (f32 always) and the ordering on `stream` are those of the f32
 * entry on the same input.  No byte outside [d_out_pcm[i], d_out_pcm[i] + out_caps[i] * out_bits / 8) is written; a capacity
 * too small is RSMP_ERR_CAPACITY before anything is launched.  Planned on the host.  Streams of two channels (f32 or PCM input)
 * or, from f32 input, of an even count of 4 .. 16 channels -- a 5.1, 7.1 or 8-channel file; the contract is the same with the
 * stream's own `channels`, and one batch may mix the counts.  Long launches need the 128-tap rate pairs of the split kernel as PCM
 * input does, at most one launch's worth of input per stream; a launch of fewer than 16384 output frames, and a rate pair without
 * a short period at any length, is served by the generic kernels -- for more than two channels the latency kernel.  Still refused: one channel, odd counts, more than 16 channels, and
 * PCM input of other than two channels (rsmp_pcm_to_stereo_f32_device reads stereo files: pass f32).  These and anything else
 * are RSMP_ERR_INVALID_ARGUMENT before any launch, with nothing written and no state changed -- take f32 output and convert with
 * rsmp_f32_to_pcm_device.
 * Dither is a setting of the handles (rsmp_fir_set_pcm_dither below, default RSMP_DITHER_NONE). */
int rsmp_fir_batch_resample_bulk_pcm_out_device(rsmp_fir* const* rs, size_t n, const void* const* d_in, int in_bits,
                                                const size_t* in_lens, size_t chunk_len, void* const* d_out_pcm, int out_bits,
                                                const size_t* out_caps, size_t* consumed, size_t* produced, void* stream);
/* Dither of the PCM the entry above writes for this handle: RSMP_DITHER_NONE (the default) or RSMP_DITHER_TPDF with the stream's
 * `seed`; anything else is RSMP_ERR_INVALID_ARGUMENT and changes nothing.  A setting, not state: it survives rsmp_fir_reset and
 * rsmp_fir_seek.  With TPDF every sum is quantised where it is stored by rsmp_f32_to_pcm_dither's rule (below), output frame n of
 * a launch and channel c with the index
 *   i = (abs_out + n) * channels + c,
 * abs_out = the output frames the handle has produced since it was made or last reset -- after rsmp_fir_seek, the plan's.  So
 * the bytes are exactly rsmp_f32_to_pcm_dither_device's of the f32 entry's output with first_index = abs_out * channels: a
 * stream's bytes do not depend on how its input is cut into launches (beyond what the f32 sums themselves do), reset starts the
 * noise sequence again, and the repair pass, which rewrites chunks with non-finite sums, gives them the noise they had.  One mode
 * for all the streams of a batch, as out_bits -- a mix is RSMP_ERR_INVALID_ARGUMENT before any launch, nothing written, no state
 * changed --; the seeds are per stream.  rsmp_fir_pcm_dither reads the setting back (either pointer may be NULL). */
int rsmp_fir_set_pcm_dither(rsmp_fir* r, int dither, uint64_t seed);
int rsmp_fir_pcm_dither(const rsmp_fir* r, int* dither, uint64_t* seed);
/* Shape of that dither: RSMP_DITHER_SHAPE_WHITE (the default: the bytes of a handle that never set it) or
 * RSMP_DITHER_SHAPE_HIGHPASS; anything else, or a null handle, is RSMP_ERR_INVALID_ARGUMENT and the setting stays.  A setting like
 * the dither mode: it survives rsmp_fir_reset and rsmp_fir_seek, and only a PCM-output launch whose dither mode is RSMP_DITHER_TPDF
 * reads it -- with RSMP_DITHER_NONE it has no effect.  The bytes, and with statistics on the totals, are exactly
 * rsmp_f32_to_pcm_shaped_device's (below) of the f32 entry's output with the handle's gain, dither, shape and seed, the stream's
 * `channels` and first_index = abs_out * channels: the first frame after a reset draws its earlier value from the wrapped index
 * 2^64 - channels + c, and a chunk the repair pass rewrites gets the noise it had.  One shape for all the streams of a batch, as the
 * dither mode and out_bits -- a mix is RSMP_ERR_INVALID_ARGUMENT before any launch: nothing written, no state changed, nothing
 * counted --; seeds and gains stay per stream.  rsmp_fir_pcm_dither_shape reads the setting back (null: RSMP_ERR_INVALID_ARGUMENT). */
int rsmp_fir_set_pcm_dither_shape(rsmp_fir* r, int shape);
int rsmp_fir_pcm_dither_shape(const rsmp_fir* r, int* shape);
/* Output gain of the PCM that entry writes for this handle, folded into the factor its stores multiply by anyway -- the rule is
 * rsmp_f32_to_pcm_gain's (below), and the bytes are exactly rsmp_f32_to_pcm_gain_device's of the f32 entry's output with the
 * handle's gain, dither, seed and first_index = abs_out * channels.  A setting, not state: the default is 1 (the bytes of a handle
 * that never set it), it survives rsmp_fir_reset and rsmp_fir_seek, and a change takes effect at the handle's next PCM-output
 * launch.  Only the PCM-output entry reads it: the f32 entries, the lock-step batch and the buffered history ignore it.  It is
 * per stream: the streams of a batch may differ in it, unlike out_bits, the dither mode and the statistics setting.  Accepted:
 * finite gains with 2^-32 <= |gain| <= 2^32, negative ones included (polarity); zero, NaN, infinities and anything outside the
 * range are RSMP_ERR_INVALID_ARGUMENT and change nothing.  With statistics on, the totals describe the gained values
 * (rsmp_f32_to_pcm_gain): a second pass at gain g reports about g times the first pass's peak.  rsmp_fir_pcm_gain reads the
 * setting back (null handle or null `gain`: RSMP_ERR_INVALID_ARGUMENT). */
int rsmp_fir_set_pcm_gain(rsmp_fir* r, float gain);
int rsmp_fir_pcm_gain(const rsmp_fir* r, float* gain);
/* Statistics of the PCM that entry writes for this handle: a setting, default 0 (off), that survives rsmp_fir_reset and
 * rsmp_fir_seek like the dither setting.  With it on, a PCM-output launch takes builds of its kernels that count every value they
 * store by rsmp_f32_to_pcm_stats's rule (below) -- the bytes are unchanged -- and adds the launch's counts to the handle's totals
 * in device memory: exactly rsmp_f32_to_pcm_stats's of the f32 entry's output with the handle's dither, seed and
 * first_index = abs_out * channels, chunks rewritten by the repair pass counted as rewritten.  One setting for all the streams of
 * a batch, as out_bits and the dither mode: a mix is RSMP_ERR_INVALID_ARGUMENT before any launch, nothing written, no state
 * changed.  Turning the setting on allocates the 32 bytes.
 * rsmp_fir_pcm_stats: the totals of every PCM-output launch of the handle since it was made, last reset or last clear; waits for
 * the handle's last launch, as rsmp_fir_last_kernel_ms does, then copies 32 bytes.  A handle with the setting off: all zero.
 * rsmp_fir_pcm_stats_clear zeroes the totals; rsmp_fir_reset and rsmp_fir_batch_reset do the same -- a new stream starts,
 * as the dither sequence does --, rsmp_fir_seek leaves them.  A clear is ordered like any other call of the handle, behind the
 * launches made before it and ahead of those made after it, and enqueues nothing: the next counting launch replaces the totals
 * instead of adding to them.  Null handle or null `stats`: RSMP_ERR_INVALID_ARGUMENT, nothing written. */
int rsmp_fir_set_pcm_stats(rsmp_fir* r, int enable);
int rsmp_fir_pcm_stats(rsmp_fir* r, rsmp_pcm_stats* stats);
int rsmp_fir_pcm_stats_clear(rsmp_fir* r);

/* reset() for every stream of a batch. */
void rsmp_fir_batch_reset(rsmp_fir* const* rs, size_t n);

/* ---- lock-step batch: a fixed set of streams, ONE resample() call per stream and step ------------
 * BASELINE config 4 (1024 mixed-rate streams, one 512-frame chunk each per step).  Per stream a step
 * is exactly ResamplerFir::resample (resampler_fir.rs:509-621) on d_in[i] + in_offset_frames*channels_i
 * (in_frames frames) into d_out[i] (or, with `append`, behind what the earlier steps wrote there): same
 * frames accepted, same output, same frames kept.  Unlike the calls above the reference's state
 * (read_position / available_frames / position, :189-192) lives in HBM and the control flow runs inside
 * the kernel, one lane per stream: a step is a single launch with constant arguments and no per-stream
 * host work, whatever states the streams are in.  Consequently the (consumed, produced) counts of a step
 * are device data: rsmp_fir_lockstep_counts waits for the last step and copies them out.
 * While a batch exists its streams must not be used through other entry points; rsmp_fir_lockstep_sync
 * (and _free) write the device state back into the handles.  out_caps[i] must be at least
 * rsmp_fir_buffer_size_output (the reference's documented sizing).  Steps of one batch are ordered. */
typedef struct rsmp_fir_lockstep rsmp_fir_lockstep;
rsmp_fir_lockstep* rsmp_fir_lockstep_new(rsmp_fir* const* rs, size_t n, size_t max_step_frames);
void rsmp_fir_lockstep_free(rsmp_fir_lockstep* ls);
size_t rsmp_fir_lockstep_size(const rsmp_fir_lockstep* ls);
size_t rsmp_fir_lockstep_workgroups(const rsmp_fir_lockstep* ls);   /* diagnostic: workgroups per step */
/* ... and how many of them use split operands on the fp16 matrix cores (two-channel streams in
 * RSMP_FIR_KERNEL_AUTO; the others keep every product in f32: other channel counts, streams set to another
 * kernel mode with rsmp_fir_set_kernel before the batch was made, geometries whose image does not fit). */
size_t rsmp_fir_lockstep_split_workgroups(const rsmp_fir_lockstep* ls);
/* Binding (again) starts the `append` positions at the front of the new output buffers.  With `append` the
 * caller sizes d_out[i] for all the steps it will run until the next bind (the kernel checks the room of one
 * step, out_caps[i], not of the buffer). */
int rsmp_fir_lockstep_bind(rsmp_fir_lockstep* ls, const float* const* d_in, float* const* d_out,
                           const size_t* out_caps);
/* d_in_frames: optional DEVICE array of frames offered per stream (in the order of `rs`; NULL = in_frames
 * for every stream; entries above max_step_frames are clamped). */
int rsmp_fir_lockstep_step(rsmp_fir_lockstep* ls, size_t in_frames, size_t in_offset_frames,
                           const uint32_t* d_in_frames, int append, void* stream);
int rsmp_fir_lockstep_counts(rsmp_fir_lockstep* ls, size_t* consumed, size_t* produced);
/* k_steps consecutive steps in one go: per stream the reference's driver loop (resample/src/main.rs:226-254) over the
 * k_steps * in_frames frames at d_in[i] + in_offset_frames, one resample() call (src/resampler_fir.rs:509-621) per
 * in_frames frames -- the same calls, counts, samples and end state as k_steps calls of rsmp_fir_lockstep_step with
 * `append` at offsets in_offset_frames + s * in_frames.  The calls are planned on the device (one lane per stream
 * replays the reference's control flow for the k_steps calls) and computed by the bulk kernels, one launch per rate
 * pair for the whole run, instead of k_steps launches of the one-call kernel.  The outputs of the calls follow each
 * other in d_out[i]: behind what was appended before (append != 0), or from the front of the buffer (append == 0: the
 * append position starts again there); the caller sizes d_out[i] for the run.  rsmp_fir_lockstep_counts returns the
 * last call's counts, rsmp_fir_lockstep_run_counts all of them: consumed[s * n + i], produced[s * n + i] for call s
 * of stream i (up to max_steps calls).  Batches with a rate pair no bulk kernel serves (irrational ratios) and runs
 * of one call are executed as a loop of steps. */
int rsmp_fir_lockstep_run(rsmp_fir_lockstep* ls, size_t k_steps, size_t in_frames, size_t in_offset_frames,
                          int append, void* stream);
int rsmp_fir_lockstep_run_counts(rsmp_fir_lockstep* ls, size_t* consumed, size_t* produced, size_t max_steps);
/* A whole buffer per stream as the reference's driver loop feeds it (resample/src/main.rs:226-254): total_frames frames
 * from d_in[i] + in_offset_frames in calls of chunk_frames frames, the last call shorter where total_frames is no
 * multiple -- floor(total / chunk) calls through rsmp_fir_lockstep_run and the remaining frames as one more call, its
 * output appended behind theirs.  Asynchronous on `stream`, planned on the device whatever states the streams are in
 * (no host planning, no host threads): the bulk entry point for batches of streams in DISTINCT states.  Counts:
 * rsmp_fir_lockstep_run_counts (the equal calls) and rsmp_fir_lockstep_counts (the last call); rsmp_fir_lockstep_sync
 * brings the streams' states back into their handles.  chunk_frames <= the batch's max_step_frames, and calls every stream
 * accepts WHOLE: chunk_frames + taps + 8 <= 4096 (INPUT_CAPACITY, resampler_fir.rs:18; the driver loop offers a call's
 * remainder again, a run's calls read at fixed offsets) -- RSMP_ERR_INVALID_INPUT_BUFFER_SIZE otherwise. */
int rsmp_fir_lockstep_run_bulk(rsmp_fir_lockstep* ls, size_t total_frames, size_t chunk_frames, size_t in_offset_frames,
                               int append, void* stream);
/* rsmp_fir_lockstep_run_bulk with a buffer length per stream: total_frames[i] frames (HOST array, the order of `rs`,
 * read before the call returns) from d_in[i] + in_offset_frames, in calls of chunk_frames frames, the stream's last call
 * shorter where total_frames[i] is no multiple -- per stream exactly the calls resample/src/main.rs:226-254 makes, no
 * others: a stream with total_frames[i] == 0 makes no call and keeps its state, counts and append position.
 * Asynchronous on `stream` and ordered like every other device entry; ALL of a stream's calls, the short one included, are
 * planned on the device in one run and computed by one launch per kernel build.  Limits as for rsmp_fir_lockstep_run_bulk:
 * chunk_frames <= max_step_frames and chunk_frames + taps + 8 <= 4096 (RSMP_ERR_INVALID_INPUT_BUFFER_SIZE otherwise), at most
 * 2^27 frames / 2^31 outputs / 2^20 calls per stream and run; the caller sizes d_out[i] for the stream's whole run, out_caps[i]
 * stays the room of ONE call.  NULL ls / total_frames or chunk_frames == 0: RSMP_ERR_INVALID_ARGUMENT (checked before anything
 * touches the device); all lengths zero: RSMP_OK, nothing enqueued.
 * Counts: with calls_i = ceil(total_frames[i] / chunk_frames), rsmp_fir_lockstep_run_counts returns max_i calls_i rows; row s
 * of stream i is its call s -- the short last call included, as row calls_i - 1 -- and (0, 0) for s >= calls_i.
 * rsmp_fir_lockstep_counts returns every stream's OWN last call (a stream without a call keeps what it had).
 * rsmp_fir_lockstep_sync_totals, _status, _run_slow_calls and _sync work as after any run.  An array of equal lengths gives
 * what rsmp_fir_lockstep_run_bulk gives: the same counts, the same end states bit for bit.
 * A ragged run is neither planned ahead nor does it keep a run that was planned ahead: the launch plans on `stream` itself, and
 * the next rsmp_fir_lockstep_run after it plans there too.  Batches with a rate pair no bulk kernel serves run as a loop of steps
 * in which a stream that is through takes empty calls (state-neutral; they appear in no count). */
int rsmp_fir_lockstep_run_bulk_v(rsmp_fir_lockstep* ls, const size_t* total_frames, size_t chunk_frames,
                                 size_t in_offset_frames, int append, void* stream);
/* Diagnostic: calls of the last run (all streams) that the device planner's fast path declined and the plain state
 * machine did (fir_mirror_fast.h); 0 for a run executed as a loop of steps. */
int rsmp_fir_lockstep_run_slow_calls(rsmp_fir_lockstep* ls, size_t* slow_calls);
/* Diagnostic: how often a class of the batch's streams was given new class tables because the streams' f64 position drift
 * (src/resampler_fir.rs:589: ~1e-14 of a frame per output, for as long as a stream runs) had moved away from the drift
 * its tables were mixed for.  The batch watches the drifts itself (an asynchronous read-back every 2^19 frames per
 * stream); nothing for the caller to do. */
int rsmp_fir_lockstep_table_rebinds(const rsmp_fir_lockstep* ls, size_t* rebinds);
/* Diagnostic counters of a batch, out[0 .. n): [0] table rebinds (as above), [1] runs taken over from the plan stream
 * (planned while the run before them computed), [2] runs planned ahead and dropped (the caller did something else),
 * [3] looks at the drifts that found a class past its tolerance with its next tables still on their way (the old ones
 * serve until the next look; a replacement is prepared by a worker thread, never inside a launch call), [4] times a
 * launch call WAITED for that worker (a class three tolerances past its tables: never observed), [5] probes of which
 * plan stream runs beside a caller's stream, [6] 1 if the last run's stream has a plan stream, [7] drift classes, [8] runs
 * taken over whose states were committed on the plan stream (batches under 256 streams, no new buffers or tables in between). */
#define RSMP_LS_STAT_COUNT 9
int rsmp_fir_lockstep_stats(const rsmp_fir_lockstep* ls, uint64_t* out, size_t n);
/* How closely the class tables follow the streams' drift: a class gets new tables when its drift is more than
 * `tolerance_frames` (default 1.2e-7: at worst 2e-7 of a full-scale sample, a fifth of the 1e-6 bound; 2e-8 .. 1e-6) from
 * what its tables were mixed for; the drifts are read back every `check_frames` input frames per stream (default 2^19).
 * Tighter = closer to the reference's phase rows, more replacements (each is prepared off the launch path). */
int rsmp_fir_lockstep_set_drift_policy(rsmp_fir_lockstep* ls, double tolerance_frames, size_t check_frames);
/* Sticky per-stream flags: 1 = more position runs in one step than the kernel keeps (outputs of that step
 * undefined; never observed), 2 = a step saw non-finite samples and was evaluated in the reference's
 * two-row form, 4 = the f64 position drifted out of the class tables' tolerance (reference form from then on),
 * 8 = a call of a run accepted fewer frames than it was offered (cannot happen below 3960 frames per step),
 * 16 = rsmp_fir_lockstep_run's planner found, replaying a call, a premise of its closed form violated (a drift of the f64
 * position beyond 1 / out_hz; never observed: the run's counts are then not the reference's). */
int rsmp_fir_lockstep_status(rsmp_fir_lockstep* ls, uint32_t* status);
int rsmp_fir_lockstep_sync(rsmp_fir_lockstep* ls);
/* rsmp_fir_lockstep_sync + what every stream has done since the batch's states were last exchanged with the handles (creation, reset,
 * the previous sync): accepted[i] = frames accepted x channels, produced[i] = frames produced x channels -- the (consumed, produced) a
 * bulk driver loop over the same input would return (resample/src/main.rs:226-254: every call accepts its whole offer) --, *status_or =
 * the OR of the streams' sticky flags.  rsmp_fir_lockstep_in_sync: *in_sync = 1 if no handle has been touched through another entry
 * point since (its state and history buffer are what the batch last wrote back): a host that alternates between the batch and other
 * entries re-creates the batch when this says 0.  rsmp_fir_batch_distinct_states: how many different states n handles are in (what a
 * host-planned bulk launch has to plan: streams in one state and fed the same amount share a plan). */
/* New buffers under a bound batch -- the same capacities, states and histories; what rsmp_fir_lockstep_bind does when only d_in / d_out
 * change, without its waits: the table goes to the device in `stream` order, and a run planned ahead (rsmp_fir_lockstep_run: the next
 * run of a caller that feeds run after run) survives if it starts at the front of the output -- the two pointers of its descriptors are
 * patched when it is taken over.  A service that hands every launch fresh buffers keeps the planner off its critical path that way. */
int rsmp_fir_lockstep_rebind_buffers(rsmp_fir_lockstep* ls, const float* const* d_in, float* const* d_out, void* stream);
/* rsmp_fir_lockstep_free without the write-back: for a batch whose handles have been used through other entry points since its last
 * sync (the handles hold the newer state). */
void rsmp_fir_lockstep_discard(rsmp_fir_lockstep* ls);
int rsmp_fir_lockstep_sync_totals(rsmp_fir_lockstep* ls, size_t* accepted, size_t* produced, uint32_t* status_or);
int rsmp_fir_lockstep_in_sync(const rsmp_fir_lockstep* ls, int* in_sync);
int rsmp_fir_batch_distinct_states(rsmp_fir* const* rs, size_t n, size_t* distinct);
/* Measurement hooks, as rsmp_fir_set_profiling / rsmp_fir_mean_kernel_ms: HIP events on the launch stream
 * around every step while enabled; the mean covers the (up to 64) most recent steps. */
int rsmp_fir_lockstep_set_profiling(rsmp_fir_lockstep* ls, int enable);
int rsmp_fir_lockstep_mean_kernel_ms(rsmp_fir_lockstep* ls, float* ms, size_t* launches);
/* ... and each of the last min(cap, 256) profiled launches' device time, oldest first (median / max of a bench) */
int rsmp_fir_lockstep_kernel_ms(rsmp_fir_lockstep* ls, float* ms, size_t cap, size_t* launches);
int rsmp_fir_lockstep_reset(rsmp_fir_lockstep* ls);   /* reset() of every stream (resampler_fir.rs:638-642) */

/* ---- host-only: filter design and the (consumed, produced) state machine ----------------------- */
/* make_sincs_for_kaiser table exactly as ResamplerFir::create_fir_coeffs lays it out
 * (resampler_fir.rs:406-422, window.rs:17-55): out[1024][taps]. */
int rsmp_design_fir_coeffs(uint32_t input_rate_hz, uint32_t output_rate_hz, int latency,
                           int attenuation, float* out, size_t out_len);
/* calculate_cutoff_kaiser (window.rs:114-131). */
double rsmp_design_cutoff_kaiser(size_t sample_count, double beta);

typedef struct rsmp_fir_plan rsmp_fir_plan;   /* host mirror of {read_position, available_frames, position} */
typedef struct {
    uint32_t out_start;   /* index of the first output frame of the run inside the launch      */
    uint32_t count;       /* output frames in the run                                          */
    int64_t in_base;      /* input frame (relative to the first buffered frame at launch start) */
                          /* that local position 0.0 refers to                                  */
    double p0;            /* position of the run's first frame (resampler_fir.rs:544)          */
    double inc;           /* exact position increment inside the run: p_k = p0 + k*inc         */
} rsmp_fir_segment;

rsmp_fir_plan* rsmp_fir_plan_new(uint32_t input_rate_hz, uint32_t output_rate_hz, int latency);
void rsmp_fir_plan_free(rsmp_fir_plan* p);
void rsmp_fir_plan_reset(rsmp_fir_plan* p);
void rsmp_fir_plan_state(const rsmp_fir_plan* p, size_t* read_position, size_t* available_frames,
                         double* position);
/* One reference resample() call in frames: how many input frames are accepted, how many output
 * frames are produced, and the exact position runs (segs may be NULL). */
int rsmp_fir_plan_call(rsmp_fir_plan* p, size_t input_frames, size_t output_capacity_frames,
                       size_t* frames_accepted, size_t* frames_produced, rsmp_fir_segment* segs,
                       size_t max_segs, size_t* n_segs);

/* A copy of the plan (its state); NULL for NULL. */
rsmp_fir_plan* rsmp_fir_plan_clone(const rsmp_fir_plan* p);
/* The driver loop of resample/src/main.rs:226-254 on the plan alone: calls of min(chunk_frames, remaining)
 * input frames with the full output capacity until in_frames are used up or max_calls calls were made
 * (0 = no limit).  Totals in frames.  What rsmp_fir_resample_bulk would do to a stream in this state. */
int rsmp_fir_plan_bulk(rsmp_fir_plan* p, size_t in_frames, size_t chunk_frames, size_t max_calls,
                       size_t* frames_accepted, size_t* frames_produced, size_t* n_calls);
/* Diagnostic: the device planner's arithmetic for runs of equal calls (rsmp_fir_lockstep_run; fir_mirror_fast.h:
 * structure predicted in exact integer arithmetic, the f64 chain verified against it) run on the host next to the
 * plain state machine for `calls` calls of in_frames frames, predicted in runs of run_len calls; compares counts,
 * every bit of the state and the outputs at integer positions call by call.  *mismatches must come back 0;
 * *slow_calls = calls the fast path declined (done by the plain state machine), *lean_calls = calls that were also done
 * by the unchecked chain the device takes where the prediction has no tie.  The plan advances by the calls. */
int rsmp_fir_plan_selftest_fast(rsmp_fir_plan* p, size_t in_frames, size_t calls, size_t run_len,
                                size_t* mismatches, size_t* slow_calls, size_t* lean_calls);
/* Starts a resampler in the middle of a stream: the handle takes the plan's state (same rate pair and
 * latency) and, as its buffered frames, the last available_frames * channels values of `history` -- the
 * input that precedes the point (host or device memory).  A stream cut at call boundaries found with
 * rsmp_fir_plan_bulk can so be resampled piece by piece, on different GPUs, with the output of one pass
 * (the reference has no counterpart: its state is private, resampler_fir.rs:189-192). */
int rsmp_fir_seek(rsmp_fir* r, const rsmp_fir_plan* p, const float* history, size_t history_len,
                  int history_on_device, void* stream);

/* ============================ CLI helpers around the path (resample/src) ========================== */
/* InterpolationResampler (resample/src/interpolation_resampler.rs:41-126): the comparison interpolators of
 * the reference's command-line tool, whole buffer in, ceil(frames * out / in) frames out. */
enum { RSMP_INTERP_LINEAR = 0, RSMP_INTERP_HERMITE = 1 };
size_t rsmp_interp_output_len(size_t channels, uint32_t in_hz, uint32_t out_hz, size_t in_len);   /* in f32 values */
int rsmp_interp_resample(int mode, size_t channels, uint32_t in_hz, uint32_t out_hz, const float* in,
                         size_t in_len, float* out, size_t out_cap, size_t* produced);
int rsmp_interp_resample_device(int mode, size_t channels, uint32_t in_hz, uint32_t out_hz, const float* d_in,
                                size_t in_len, float* d_out, size_t out_cap, size_t* produced, void* stream);
/* WAV sample conversion of the tool (resample/src/main.rs:128-156): little-endian integer PCM (16, packed
 * 24, 32 bits) -> f32 = s / 2^(bits-1), mono duplicated to both channels; d_out holds n_samples values
 * (2 channels in) or 2 * n_samples (1 channel in).  Device pointers, asynchronous on `stream`. */
int rsmp_pcm_to_stereo_f32_device(const void* d_pcm, int bits, int channels, size_t n_samples, float* d_out,
                                  void* stream);
/* The way back, f32 -> little-endian integer PCM of `bits` (16, packed 24, 32), n_values * bits / 8 bytes:
 *   q = saturate(round_half_to_even(x * 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1),  NaN -> 0.
 * The product is exact (a power of two); +inf and everything above the range give the top code, -inf and everything below the
 * bottom one, -0.0 and denormals 0; +1.0 saturates to the top code.  No dither here (rsmp_f32_to_pcm_dither below; its high-pass
 * form: rsmp_f32_to_pcm_shaped), no error-feedback noise shaping.  Decoding with
 * rsmp_pcm_to_stereo_f32_device and quantising again at the same width is the identity on every 16-bit and 24-bit code.  At 32
 * bits it is NOT: the reference decodes 32-bit files with the divisor -2^31 (resample/src/main.rs:131), the scale here is
 * +2^31 -- an f32 value means what it says --, so that round trip gives saturate(-f32(s)): polarity inverted, the bottom code
 * saturated to the top one.
 * rsmp_f32_to_pcm: host memory, needs no device -- the definition itself.  rsmp_f32_to_pcm_device: device pointers,
 * asynchronous on `stream`; d_in 16-byte aligned, d_pcm 4-byte aligned, any n_values; writes exactly n_values * bits / 8 bytes. */
int rsmp_f32_to_pcm(const float* in, size_t n_values, int bits, void* out_pcm);
int rsmp_f32_to_pcm_device(const float* d_in, size_t n_values, int bits, void* d_pcm, void* stream);
/* The same with dither.  RSMP_DITHER_NONE: the bytes of rsmp_f32_to_pcm.  RSMP_DITHER_TPDF: value j of the call has the absolute
 * index i = first_index + j (wrapping, 64 bits) and is quantised as
 *   q = saturate(round_half_to_even(f32(x * 2^(bits-1)) + d(seed, i))),  NaN -> 0:
 * ONE f32 addition behind the exact product (an fma of the same operands gives the same bits); saturation, infinities and NaN
 * as above.  The noise has no state -- it is a function of the seed and the index (arithmetic mod 2^64, splitmix64):
 *   z = seed + ((i >> 1) + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB;          w = z ^ z >> 31;
 *   h = low 32 bits of w for even i, high 32 bits for odd i;  r1 = h & 0xFFFF, r2 = h >> 16;  d = f32(r1 - r2) * 2^-16
 * -- the difference of two uniform 16-bit numbers: triangular on (-1, 1) LSB, variance 1/6, the usual TPDF dither; the error
 * of the result has mean zero and a variance that does not depend on the signal.  This noise is spectrally white; its high-pass
 * form, with the same density and variance, is RSMP_DITHER_SHAPE_HIGHPASS (rsmp_f32_to_pcm_shaped).  One mix serves two consecutive values, one
 * two-channel frame.  Converting a buffer in pieces, each with first_index advanced by the values before it, gives the bytes of
 * one call.  Unknown modes are RSMP_ERR_INVALID_ARGUMENT.  Host / device versions, pointers and alignment as above. */
int rsmp_f32_to_pcm_dither(const float* in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                           void* out_pcm);
int rsmp_f32_to_pcm_dither_device(const float* d_in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                                  void* d_pcm, void* stream);
/* The same, and what it did.  For a value x (before scaling), width `bits` and noise d (0 without dither) let
 *   v = round_half_to_even(f32(x * 2^(bits-1)) + d)   -- the quantiser's own v.  Then
 *   values   counts every value;
 *   nans     those with x NaN (stored as 0, not clipped);
 *   clipped  those with v not NaN and outside the code range: v > 2^(bits-1) - 1 or v < -2^(bits-1); at 32 bits, whose top code is
 *            no f32 value, v >= 2^31 or v < -2^31.  So +-inf clip, +1.0 clips, -1.0 does not;
 *   peak     the maximum of |x| over the values that are not NaN, an f32, before scaling and before dither (+inf possible; 0.0
 *            when there is no such value).
 * No field depends on the order of evaluation.  The bytes written are rsmp_f32_to_pcm_dither[_device]'s with the same arguments;
 * out_pcm / d_pcm may be NULL: measure only.  Host version (needs no device: the definition): *stats is OVERWRITTEN.  Device
 * version (asynchronous on `stream`): the call's statistics are MERGED into *d_stats -- device memory, 8-byte aligned, zeroed by the
 * caller --, so a buffer converted in pieces, each with first_index advanced, accumulates the statistics of one call.  Unknown
 * `bits` or `dither`, null `stats`: RSMP_ERR_INVALID_ARGUMENT, nothing written. */
int rsmp_f32_to_pcm_stats(const float* in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                          void* out_pcm, rsmp_pcm_stats* stats);
int rsmp_f32_to_pcm_stats_device(const float* d_in, size_t n_values, int bits, int dither, uint64_t seed, uint64_t first_index,
                                 void* d_pcm, rsmp_pcm_stats* d_stats, void* stream);
/* The same under an output gain: what the fused PCM stores of both engines do (rsmp_fir_set_pcm_gain, rsmp_fft_set_pcm_gain),
 * as a pass of its own.  For a value x with absolute index i, width `bits`, noise d (0 without dither):
 *   k = f32(gain) * 2^(bits-1)              (exact: a power-of-two multiple of an f32; a normal f32 for every accepted gain)
 *   p = f32(x * k)                          (one rounding)
 *   q = saturate(round_half_to_even(f32(p + d(seed, i)))),  p NaN -> 0
 * -- the product and the sum are two operations (no fma: for a gain that is no power of two it would round once and give other
 * bytes); i, d, saturation and the 32-bit top code as above.  With gain == 1, k is 2^(bits-1) and the bytes are
 * rsmp_f32_to_pcm_dither's for every input.
 * Accepted gains: finite, 2^-32 <= |gain| <= 2^32, negative ones included (polarity).  Zero, NaN, infinities and anything outside
 * the range: RSMP_ERR_INVALID_ARGUMENT, nothing written.
 * Consequence: for a power-of-two gain the bytes equal rsmp_f32_to_pcm[_dither]'s of x * gain; for any gain they equal its bytes
 * of f32(x * gain) wherever |x * gain| >= 2^-126 (both products then round at the same bit); below that both give code 0 without
 * dither.
 * The statistics describe what was quantised: nans counts p NaN; clipped goes by v = round_half_to_even(f32(p + d)), as above;
 * peak is the largest |p| * 2^-(bits-1), computed in f32 -- the peak of the gained signal, so a second pass at gain g reports
 * about g times the first pass's peak.  With gain 1 it is rsmp_f32_to_pcm_stats's |x|, except that an x whose product
 * x * 2^(bits-1) overflows f32 (|x| >= 2^(129-bits)) counts as +inf here.
 * Host version (needs no device: the definition): `stats` may be NULL, else *stats is OVERWRITTEN.  Device version: alignment and
 * ordering as rsmp_f32_to_pcm_stats_device, the statistics MERGED into *d_stats, which may be NULL too.  out_pcm / d_pcm may be
 * NULL where statistics are taken: measure only. */
int rsmp_f32_to_pcm_gain(const float* in, size_t n_values, int bits, float gain, int dither, uint64_t seed, uint64_t first_index,
                         void* out_pcm, rsmp_pcm_stats* stats);
int rsmp_f32_to_pcm_gain_device(const float* d_in, size_t n_values, int bits, float gain, int dither, uint64_t seed,
                                uint64_t first_index, void* d_pcm, rsmp_pcm_stats* d_stats, void* stream);
/* rsmp_f32_to_pcm_gain with a shape of the TPDF noise (RSMP_DITHER_SHAPE_*) and the channel count of the interleaved buffer:
 * what the fused PCM stores do under rsmp_fir_set_pcm_dither_shape / rsmp_fft_set_pcm_dither_shape.  With h(seed, i) the 32 bits
 * rsmp_f32_to_pcm_dither gives value i, r1(i) = h & 0xFFFF and r2(i) = h >> 16:
 *   RSMP_DITHER_SHAPE_WHITE     d = f32(r1(i) - r2(i)) * 2^-16             -- unchanged: bytes and statistics are
 *                                                                             rsmp_f32_to_pcm_gain's for every input;
 *   RSMP_DITHER_SHAPE_HIGHPASS  d = f32(r1(i) - r1(i - channels)) * 2^-16  -- i - channels wraps in 64 bits: value i < channels
 *                                                                             draws from index 2^64 - channels + i.
 * Value j of the call has index i = first_index + j and belongs to channel i % channels; only the lag depends on `channels`
 * (>= 1).  The high-pass noise is u[n] - u[n-1] of one uniform sequence per channel: the same triangular density on (-1, 1) LSB
 * and the same variance 1/6 as white, the error's first two moments independent of the signal, consecutive values of a channel
 * correlated by -1/2 and no others, so that the noise power follows 1 - cos(w) times the white level: nothing at DC, twice the
 * white level at Nyquist, 0.0064 of it in the lowest sixteenth of the band.  No error feedback: the noise has no state, and
 * converting a buffer in pieces, each with first_index advanced by the values before it, gives the bytes of one call -- pieces may
 * end inside a frame.  Everything around d -- k, the one rounding of x * k, the one f32 addition, rounding, saturation, NaN, the
 * statistics -- is rsmp_f32_to_pcm_gain's; with RSMP_DITHER_NONE the shape has no effect (it must still be a known one).
 * Pointers, alignment, NULL stats / out_pcm and the merged device statistics as rsmp_f32_to_pcm_gain[_device].  Unknown bits,
 * dither or shape, channels == 0, a gain outside the range: RSMP_ERR_INVALID_ARGUMENT, nothing written. */
int rsmp_f32_to_pcm_shaped(const float* in, size_t n_values, int bits, float gain, int dither, int shape, uint32_t channels,
                           uint64_t seed, uint64_t first_index, void* out_pcm, rsmp_pcm_stats* stats);
int rsmp_f32_to_pcm_shaped_device(const float* d_in, size_t n_values, int bits, float gain, int dither, int shape, uint32_t channels,
                                  uint64_t seed, uint64_t first_index, void* d_pcm, rsmp_pcm_stats* d_stats, void* stream);
/* The gain that brings a first pass's peak to target_peak in a second pass: *gain = f32(target_peak / stats->peak).
 * RSMP_ERR_INVALID_ARGUMENT, *gain untouched, when the peak is 0 or not finite, when the result is no accepted gain, or for a null
 * pointer.  The second pass's peak is target_peak to within two f32 roundings (the quotient and the product). */
int rsmp_pcm_normalise_gain(const rsmp_pcm_stats* stats, float target_peak, float* gain);
/* Batched converters: the two directions above over MANY buffers in ONE launch, each buffer -- a "stream" -- with its own length,
 * seed, first index, gain, channel count and statistics block.  What every PCM entry that refuses a launch points to (take f32 and
 * convert) then costs one launch per batch, not one per stream: FIR streams of 1, 3 or 5 channels, ResamplerFft launches the pair
 * kernel does not serve, every lock-step step or run, PCM input of any channel count.
 * One stream of a batched conversion; 64 bytes; host memory, copied by the call. */
typedef struct rsmp_pcm_batch_item {
    const void*     src;          /* device. to PCM: f32, 16-byte aligned.  to f32: PCM, 4-byte aligned */
    void*           dst;          /* device. to PCM: 4-byte aligned; may be NULL where stats != NULL (measure only).  to f32: 16-byte aligned */
    uint64_t        n_values;     /* frames * channels; 0: the stream is skipped, src / dst may be NULL */
    uint64_t        seed;         /* TPDF */
    uint64_t        first_index;  /* index of the stream's value 0 (wraps in 64 bits) */
    rsmp_pcm_stats* stats;        /* device, 8-byte aligned, or NULL; the call's statistics are MERGED into it */
    float           gain;         /* rsmp_f32_to_pcm_gain's rule and range; 1 = none */
    uint32_t        channels;     /* >= 1; only the high-pass lag reads it */
    uint64_t        reserved;     /* 0 */
} rsmp_pcm_batch_item;
/* The handle owns the descriptor tables of its calls -- a small ring of pinned host tables and their device twins, each of
 * max_streams entries (1 .. 2^24), ordered by events -- and knows its device's size.  NULL + rsmp_last_error() on failure.  Not
 * thread-safe.  rsmp_pcm_batch_free waits for the handle's launches that still read a table, and takes NULL. */
typedef struct rsmp_pcm_batch rsmp_pcm_batch;
rsmp_pcm_batch* rsmp_pcm_batch_new(size_t max_streams, int device);
void rsmp_pcm_batch_free(rsmp_pcm_batch* b);
/* f32 -> PCM.  For every stream the bytes are exactly those of rsmp_f32_to_pcm_shaped over the stream's n_values values with its
 * gain, seed, first_index and channels and the call's bits, dither and shape; exactly n_values * bits / 8 bytes are written per
 * stream and none outside.  Where stats != NULL, that function's statistics of the stream are MERGED into *stats by the rule of
 * rsmp_f32_to_pcm_stats_device (zeroed by the caller; two items may name one block); dst may then be NULL: measure only.
 * Streams without a block are not counted at all, and a batch without any runs kernels that cannot count.
 * Asynchronous on `stream`; `items` may be changed or freed when the call returns; calls on one handle may follow each other on
 * the same or on different streams without a host wait (the host waits only when more calls than the ring has tables -- four --
 * are in flight).  Buffers of one call must not overlap.
 * RSMP_ERR_INVALID_ARGUMENT, decided before anything is enqueued and with nothing written: a null handle; null items with n > 0;
 * n > max_streams; unknown bits, dither or shape; a gain outside the accepted range; channels == 0; reserved != 0; a misaligned
 * pointer, src == NULL, or dst == NULL without stats, where n_values > 0; a batch of more than 2^32 - 1 tiles
 * (rsmp_pcm_batch_tile_values).  n == 0, or every stream empty: RSMP_OK without a launch. */
int rsmp_pcm_batch_f32_to_pcm_device(rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, int dither, int shape,
                                     void* stream);
/* PCM -> f32.  Reads src, dst and n_values (and reserved, which must be 0); stats must be NULL.  Sample j of a stream becomes
 * s / 2^(bits-1), with the reference's divisor -2^31 at 32 bits (resample/src/main.rs:131) -- the value the fused PCM-input loads
 * give, bit-equal to rsmp_pcm_to_stereo_f32_device for two channels and to rsmp_pcm_to_f32.  It decodes samples, whatever the
 * channel count: no mono duplication.  Ordering and refusals as above. */
int rsmp_pcm_batch_pcm_to_f32_device(rsmp_pcm_batch* b, const rsmp_pcm_batch_item* items, size_t n, int bits, void* stream);
/* Diagnostics: the values of one tile of the batched converters (a multiple of 4; a tile never holds values of two streams), and
 * the grid of the handle's last accepted call: its workgroups and the tiles they shared (0, 0 where nothing was launched).  A
 * counting launch issues at most 4 x (workgroups + stream changes seen by workgroups) atomics.  Either pointer may be NULL. */
size_t rsmp_pcm_batch_tile_values(void);
int rsmp_pcm_batch_last_grid(const rsmp_pcm_batch* b, uint32_t* workgroups, uint64_t* tiles);
/* The decoder's definition: host memory, needs no device.  n_samples little-endian samples of `bits` (16, packed 24, 32) ->
 * out[j] = f32(s) / 2^(bits-1), the divisor -2^31 at 32 bits.  Unknown bits or a null buffer with n_samples > 0:
 * RSMP_ERR_INVALID_ARGUMENT. */
int rsmp_pcm_to_f32(const void* pcm, size_t n_samples, int bits, float* out);
/* Measurement aid (no counterpart in the reference): a plain streaming copy of n_values floats, 16 bytes per lane --
 * the rate a kernel that reads as much as it writes can reach on this GPU; bench.py reports it next to every
 * roofline fraction.  16-byte aligned device pointers, n_values a multiple of 4, asynchronous on `stream`. */
int rsmp_device_stream_copy(const float* d_src, float* d_dst, size_t n_values, void* stream);

/* ============================ ResamplerFft (src/resampler_fft.rs) =============================== */
typedef struct rsmp_fft rsmp_fft;

/* ResamplerFft::new (resampler_fft.rs:75-119); rates are SampleRate enum values.  NULL on
 * failure.  Channels are processed independently ("reference quirks"). */
rsmp_fft* rsmp_fft_new(size_t channels, int input_rate, int output_rate, int device);
void rsmp_fft_free(rsmp_fft* r);
/* ResamplerFft::chunk_size_input / chunk_size_output (resampler_fft.rs:135-145). */
size_t rsmp_fft_chunk_size_input(const rsmp_fft* r);
size_t rsmp_fft_chunk_size_output(const rsmp_fft* r);
/* ResamplerFft::delay (resampler_fft.rs:151-153). */
size_t rsmp_fft_delay(const rsmp_fft* r);
size_t rsmp_fft_channels(const rsmp_fft* r);
int rsmp_fft_set_profiling(rsmp_fft* r, int enable);
int rsmp_fft_last_kernel_ms(rsmp_fft* r, float* ms);

/* ResamplerFft::resample (resampler_fft.rs:182-240): one chunk; in_len >= chunk_size_input and
 * out_len >= chunk_size_output, extra values ignored (:186-192).  Host buffers, synchronous. */
int rsmp_fft_resample(rsmp_fft* r, const float* in, size_t in_len, float* out, size_t out_len);
int rsmp_fft_resample_device(rsmp_fft* r, const float* d_in, size_t in_len, float* d_out,
                             size_t out_len, void* stream);
/* n_chunks back-to-back chunks == n_chunks consecutive resample() calls (the whole-chunk loop of
 * resample_batch, resample/src/main.rs:276-289), one launch. */
int rsmp_fft_resample_bulk(rsmp_fft* r, const float* in, size_t in_len, float* out, size_t out_len,
                           size_t n_chunks);
int rsmp_fft_resample_bulk_device(rsmp_fft* r, const float* d_in, size_t in_len, float* d_out,
                                  size_t out_len, size_t n_chunks, void* stream);
/* n instances with the same rate pair on one device, one launch. */
int rsmp_fft_batch_resample_bulk_device(rsmp_fft* const* rs, size_t n, const float* const* d_in,
                                        float* const* d_out, const size_t* n_chunks, void* stream);
/* The same over WAV samples as they sit in the file (resample/src/main.rs:128-137): d_pcm[i] = little-endian PCM of `bits`
 * (16 / 24 / 32) per sample, two channels a frame, n_chunks[i] * chunk_size_input samples; converted inside the kernel's
 * first load (`sample as f32 / (1 << (bits - 1)) as f32`, with the reference's 32-bit divisor -2^31) -- bit for bit what
 * rsmp_pcm_to_stereo_f32_device + rsmp_fft_batch_resample_bulk_device give, one pass over HBM less.  Two-channel streams
 * of the rate pairs the wave kernel serves (72 of the 90); RSMP_ERR_INVALID_ARGUMENT otherwise.  Alignment of d_pcm[i]:
 * 8 / 4 / 16 bytes for 16 / 24 / 32 bits. */
int rsmp_fft_batch_resample_bulk_pcm_device(rsmp_fft* const* rs, size_t n, const void* const* d_pcm, int bits,
                                            float* const* d_out, const size_t* n_chunks, void* stream);
/* The other half of a file-to-file pipeline: the output as a WAV file stores it, written by the kernel's own store.  d_in[i] is
 * interleaved f32 (in_bits = 0) or PCM of in_bits (16 / 24 / 32), aligned as for rsmp_fft_batch_resample_bulk_pcm_device.
 * d_out_pcm[i], 4-byte aligned, receives exactly n_chunks[i] * chunk_size_output * out_bits / 8 bytes of little-endian PCM of
 * `out_bits` (16 / 24 / 32; 24-bit packed at 3 bytes a sample); no byte outside that range is written.  Every value the f32
 * entry would have stored is quantised where the kernel stores it (the rule: rsmp_f32_to_pcm above -- round half to even,
 * saturate, NaN -> 0), so for a handle in the same state, the same n_chunks and the same batch the bytes are exactly
 * rsmp_f32_to_pcm_device's of rsmp_fft_batch_resample_bulk_device's output, and the f32 never reaches HBM.  The overlap
 * state stays f32 and ends bit-equal to the f32 entry's.
 * Served: what the two-channel pair kernel serves -- two-channel streams of one of its 19 rate pairs (44.1 <-> 48 kHz,
 * 48 <-> 96 kHz ...), at least 4 chunks in the batch's longest stream, the default library (not libresampler_amd_fftexact.so).
 * Everything else -- other channel counts, other rate pairs, fewer than 4 chunks, the exact build, out_bits not 16 / 24 / 32,
 * null arguments, misalignment, a mix of dither modes or of statistics settings -- is RSMP_ERR_INVALID_ARGUMENT before any
 * launch: nothing is written, no state, no counter and no total changes; take f32 output and convert with rsmp_f32_to_pcm_device.
 * Dither is a setting of the handles (rsmp_fft_set_pcm_dither below, default RSMP_DITHER_NONE), and so are the statistics of
 * what this store did (rsmp_fft_set_pcm_stats below, default off). */
int rsmp_fft_batch_resample_bulk_pcm_out_device(rsmp_fft* const* rs, size_t n, const void* const* d_in, int in_bits,
                                                void* const* d_out_pcm, int out_bits, const size_t* n_chunks, void* stream);
/* Dither of the PCM the entry above writes for this handle: RSMP_DITHER_NONE (the default) or RSMP_DITHER_TPDF with the stream's
 * `seed`; anything else is RSMP_ERR_INVALID_ARGUMENT and changes nothing.  With TPDF every value is quantised where it is stored
 * by rsmp_f32_to_pcm_dither's rule, output frame n of a launch and channel c with the index
 *   i = (abs_out + n) * channels + c,
 * abs_out = the output frames the handle has produced since it was made, through ANY entry (every call that advances the
 * overlap state advances it).  So the bytes are exactly rsmp_f32_to_pcm_dither_device's of the f32 entry's output with
 * first_index = abs_out * channels, and a stream's bytes do not depend on how it is cut into launches.  ResamplerFft has no
 * reset: the noise sequence of a handle never starts again.  One mode for all the streams of a batch -- a mix is
 * RSMP_ERR_INVALID_ARGUMENT before any launch --; the seeds are per stream.  rsmp_fft_pcm_dither reads the setting back (either
 * pointer may be NULL). */
int rsmp_fft_set_pcm_dither(rsmp_fft* r, int dither, uint64_t seed);
int rsmp_fft_pcm_dither(const rsmp_fft* r, int* dither, uint64_t* seed);
/* Shape of that dither: rsmp_fir_set_pcm_dither_shape's twin, the rule rsmp_f32_to_pcm_shaped's with channels = 2 and
 * first_index = abs_out * 2.  Default RSMP_DITHER_SHAPE_WHITE; read only by a PCM-output launch whose dither mode is
 * RSMP_DITHER_TPDF; one shape for all the streams of a batch (a mix: RSMP_ERR_INVALID_ARGUMENT before any launch); an unknown shape
 * or a null handle is RSMP_ERR_INVALID_ARGUMENT and the setting stays. */
int rsmp_fft_set_pcm_dither_shape(rsmp_fft* r, int shape);
int rsmp_fft_pcm_dither_shape(const rsmp_fft* r, int* shape);
/* Output gain of the PCM that entry writes for this handle: rsmp_fir_set_pcm_gain's twin, the rule rsmp_f32_to_pcm_gain's.  The
 * bytes are exactly rsmp_f32_to_pcm_gain_device's of the f32 entry's output with the handle's gain, dither, seed and
 * first_index = abs_out * 2; with statistics on, the totals describe the gained values.  A setting with default 1, per stream
 * (a batch may mix gains), read at every PCM-output launch and by nothing else; the accepted gains and the refusals are the same. */
int rsmp_fft_set_pcm_gain(rsmp_fft* r, float gain);
int rsmp_fft_pcm_gain(const rsmp_fft* r, float* gain);
/* Statistics of the PCM that rsmp_fft_batch_resample_bulk_pcm_out_device writes for this handle: the twins of
 * rsmp_fir_set_pcm_stats / rsmp_fir_pcm_stats / rsmp_fir_pcm_stats_clear.
 * The setting belongs to the handle, is off by default and stays until it is changed (ResamplerFft has no reset).  Turning it on
 * the first time allocates the handle's totals, one rsmp_pcm_stats of 32 bytes in device memory, zeroed.
 * With the setting on, a launch through rsmp_fft_batch_resample_bulk_pcm_out_device counts every value it stores by
 * rsmp_f32_to_pcm_stats's rule and merges the counts into the totals: they are exactly rsmp_f32_to_pcm_stats's of the f32
 * entry's output for the same state, n_chunks and batch, with the handle's dither mode, its seed and first_index = abs_out * 2.
 * Counts add over launches, the peak is the larger one.  The bytes written do not change, the overlap state ends bit-equal to
 * the f32 entry's and abs_out advances as before.  Never counted: the block before its run that a wave recomputes and does not
 * store; a stream with 0 chunks in the launch (its totals stay); anything the f32-output entries produce (they advance abs_out as
 * they always did).  One setting for all the streams of a batch: a mix is RSMP_ERR_INVALID_ARGUMENT before any launch, nothing
 * written, counted or changed -- as is every request the entry refuses with the setting off.
 * rsmp_fft_pcm_stats waits for the handle's last launch through that launch's event -- not through the caller's stream, which
 * may no longer exist -- and copies the 32 bytes; with the setting off it gives all zero.  A null handle or a null `stats` is
 * RSMP_ERR_INVALID_ARGUMENT and nothing is written.
 * rsmp_fft_pcm_stats_clear is ordered like a call of the handle and enqueues nothing itself: the handle's next counting launch
 * starts from zero (it zeroes the totals on its own stream in front of its kernel), and rsmp_fft_pcm_stats between the clear and
 * that launch gives zeros. */
int rsmp_fft_set_pcm_stats(rsmp_fft* r, int enable);
int rsmp_fft_pcm_stats(rsmp_fft* r, rsmp_pcm_stats* stats);
int rsmp_fft_pcm_stats_clear(rsmp_fft* r);

/* host-only: block sizes and the N/2-point Stockham stage lists for a rate pair
 * (planner.rs:35-245, optimizer.rs:6-64, radix_fft.rs:222-246). */
int rsmp_fft_plan_sizes(uint32_t input_rate_hz, uint32_t output_rate_hz, size_t* fft_size_input,
                        size_t* fft_size_output, int* forward_stages, size_t* n_forward_stages,
                        int* inverse_stages, size_t* n_inverse_stages, size_t max_stages);

#ifdef __cplusplus
}
#endif
#endif
