/* rodio_hip.h -- C ABI of the MI355X (gfx950) implementation of rodio's per-sample DSP hot path.
 *
 * rodio has no FFI: its extension point is the Rust trait `Source: Iterator<Item = f32>`
 * (/root/reference/src/source/mod.rs:179-218).  This header is the boundary a Rust shim
 * (`struct GpuSource<I: Source>` / `GpuMixer`) binds with `extern "C"`:
 * the shim pre-pulls a block of samples from the upstream iterator, hands it to one of the
 * block functions below and serves `next()` from the returned block.  Every entry point cites
 * the reference iterator it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - Audio is interleaved f32 (`Sample = f32`, src/common.rs:36,48; src/source/mod.rs:131-135).
 *   - All data pointers are DEVICE pointers owned by the caller unless the name ends in _host.
 *     Small parameter arrays (gains, coefficients) are HOST pointers and are copied by value.
 *     Every host array of an entry that takes a stream (tables of sources, addresses, starts, lengths, segments, pairs,
 *     coefficients, parameter structures) is read before the call returns: the caller may rewrite it at once, whatever is still
 *     queued on the stream.  The one exception is a page-locked block given to rh_memcpy_h2d / rh_memcpy_h2d_rows (see there).
 *     (tests/test_gpu_stream_order.py: every such array overwritten behind the call while the stream is held back.)
 *   - Every function enqueues on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and returns an rh_status; nothing throws or aborts.  End of stream (`None`) is
 *     expressed through returned lengths, never through an error.
 *   - One handle is used from one thread at a time (mirrors `Send + !Sync`).
 *   - The one-row entries (rh_convert_*, rh_wav_decode*, rh_channels_convert, rh_amplify .. rh_take_duration_from, rh_channel_volume,
 *     rh_amplify_steps, rh_channel_volume_steps, rh_delay, rh_echo_mix, rh_resample_linear, rh_mix_sum, rh_mix_pair, rh_noise_generate)
 *     take rows (dst, src, a step table) at any address that is a multiple of the element size, and the sample bytes of
 *     rh_wav_decode* at any byte address.  Their kernels may READ the aligned 16-byte vectors that hold a row's first and last
 *     element -- up to 15 bytes either side of the row, never outside the 16 bytes that hold one of its elements, so never outside
 *     its memory page -- and nothing read there reaches a result.  They store nothing outside dst and nothing behind the count an
 *     entry reports (*out_samples); a call refused for its arguments (RH_ERR_INVALID, RH_ERR_UNSUPPORTED) has written nothing to
 *     dst.  (tests/test_gpu_arena_rows.py, tests/test_gpu_arena_formats.py: every row between NaN poison or two byte fills.)
 *   - There is NO CPU fallback: without a usable HIP device rh_init() fails and every other
 *     call returns RH_ERR_NOT_INITIALIZED / RH_ERR_HIP.
 */
#ifndef RODIO_HIP_H
#define RODIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t rh_status;
enum {
    RH_OK = 0,
    RH_ERR_INVALID = 1,         /* bad argument (zero rate/channels: rodio's NonZero types) */
    RH_ERR_HIP = 2,             /* a HIP runtime call failed; see rh_last_hip_error() */
    RH_ERR_UNSUPPORTED = 3,     /* valid in rodio, not covered by this kernel set */
    RH_ERR_NOMEM = 4,
    RH_ERR_TIMEOUT = 5,         /* an in-kernel bounded wait expired (fused pipeline) */
    RH_ERR_NOT_INITIALIZED = 6,
    RH_ERR_CAPACITY = 7         /* output buffer too small */
};

typedef void *rh_stream; /* hipStream_t */

/* ---- runtime ------------------------------------------------------------------------- */
int32_t rh_version(void);
const char *rh_status_string(rh_status s);
const char *rh_last_hip_error(void);
/* Binds the library to a gfx950 device.  Also (re-)reads the library's diagnostic / tuning environment variables (DESIGN.md
 * 7.1): nothing reads the environment on a call's way to a launch. */
rh_status rh_init(int32_t device);
rh_status rh_device_name(char *buf, size_t cap);
/* Makes the device rh_init() bound current on the CALLING thread.  HIP's current device is per thread: a helper thread of the host
 * (the reaper that frees retired streams, the pool that pulls sources) calls this once before its first call into the library, so
 * that what it frees, records or synchronises belongs to the right device in a multi-GPU process. */
rh_status rh_bind_thread(void);
/* The handle-less time-parallel kernels (rh_limit, rh_biquad mode 1) wait for hand-offs between their tiles with a bound.
 * A wait that expires (never seen on a healthy device) poisons the tile with NaN and sets a sticky word on the device:
 * RH_ERR_TIMEOUT here, once, then RH_OK again.  Covers the launches that have COMPLETED (synchronise the stream or an event
 * recorded behind them first); does not wait for anything itself.  (Handles have their own: rh_rlm_last_status.)  One word per
 * device (the one rh_init last bound), shared by every chain on it: the call that reads it first gets the report. */
rh_status rh_async_status(void);
rh_status rh_malloc(void **out, size_t bytes);
rh_status rh_free(void *p);
rh_status rh_memset(void *p, int32_t value, size_t bytes, rh_stream stream);
/* Host blocks of the two uploads: a page-locked block (rh_host_alloc) is read when `stream` reaches the copy, so it stays untouched
 * until then, and the call never waits.  A pageable block is read before the call returns, and the call may wait for it. */
rh_status rh_memcpy_h2d(void *dst, const void *src_host, size_t bytes, rh_stream stream);
/* `rows` rows of `width_bytes` each, `pitch_bytes` apart on both sides: a block of staged rows without the unused ends.
 * From a pageable block this call waits until `stream` has run everything queued before it (the runtime's pitched copy does). */
rh_status rh_memcpy_h2d_rows(void *dst, const void *src_host, size_t pitch_bytes, size_t width_bytes, size_t rows, rh_stream stream);
/* Waits until `stream` has run the copy: the host block holds the data when the call returns. */
rh_status rh_memcpy_d2h(void *dst_host, const void *src, size_t bytes, rh_stream stream);
/* For a pull-model shim (include/rodio_hip.hpp): page-locked host blocks, copies that do not synchronise. */
rh_status rh_memcpy_d2h_async(void *dst_host, const void *src, size_t bytes, rh_stream stream);
rh_status rh_memcpy_d2d(void *dst, const void *src, size_t bytes, rh_stream stream);
rh_status rh_host_alloc(void **out, size_t bytes);
rh_status rh_host_free(void *p);
rh_status rh_stream_create(rh_stream *out);
rh_status rh_stream_destroy(rh_stream s);
rh_status rh_stream_synchronize(rh_stream s);
/* The scan kernels (rh_limit, rh_biquad mode 1, rh_agc) keep a scratch buffer per stream, grown on demand and reused by every
 * later launch on that stream (rh_noise_generate and rh_crossfade use it too).  The call that makes it grow synchronises the
 * stream first: a first call of a larger shape waits, the calls after it do not.  rh_stream_destroy frees the buffer for the
 * library's own streams.  For a stream of the caller's (a PyTorch stream, ...) that is about to be destroyed: synchronises it and
 * frees its buffer (a handle value the runtime recycles must not inherit one). */
rh_status rh_stream_release_scratch(rh_stream s);
/* HIP-event timing on `stream` (bench.py measures the kernels on the stream they run on). */
rh_status rh_event_create(void **out);
rh_status rh_event_destroy(void *ev);
rh_status rh_event_record(void *ev, rh_stream stream);
rh_status rh_event_synchronize(void *ev);
/* Work queued on `stream` after this call starts once the work recorded by `ev` has completed (no host wait). */
rh_status rh_stream_wait_event(rh_stream stream, void *ev);
rh_status rh_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */

/* ---- SampleTypeConverter ("DataConverter") ---------------------------------------------
 * src/conversions/sample.rs:42-44 -> dasp_sample 0.11.0 `ToSample` (Cargo.lock:317-318).
 * Call sites: src/decoder/wav.rs:119-136, src/stream.rs:538-545 (egress).  Bit-exact. */
rh_status rh_convert_i8_to_f32(float *dst, const int8_t *src, size_t n, rh_stream stream);
rh_status rh_convert_u8_to_f32(float *dst, const uint8_t *src, size_t n, rh_stream stream);
rh_status rh_convert_i16_to_f32(float *dst, const int16_t *src, size_t n, rh_stream stream);
rh_status rh_convert_u16_to_f32(float *dst, const uint16_t *src, size_t n, rh_stream stream);
rh_status rh_convert_i24_to_f32(float *dst, const int32_t *src, size_t n, rh_stream stream); /* I24 in i32 */
rh_status rh_convert_i32_to_f32(float *dst, const int32_t *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_i8(int8_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_i16(int16_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_u16(uint16_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_i32(int32_t *dst, const float *src, size_t n, rh_stream stream);
/* The rest of cpal's device formats (src/stream.rs:555-568 egress, src/microphone.rs:280-291 ingress).
 * I24 / U24 travel in 32-bit containers like cpal's (unchecked: f32 1.0 -> I24 8388608); unsigned
 * formats go through the signed one (dasp `iN::to_uN`).  64-bit formats lose nothing that f32 has. */
rh_status rh_convert_f32_to_u8(uint8_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_i24(int32_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_u24(int32_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_u32(uint32_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_i64(int64_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_u64(uint64_t *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_f32_to_f64(double *dst, const float *src, size_t n, rh_stream stream);
rh_status rh_convert_u24_to_f32(float *dst, const int32_t *src, size_t n, rh_stream stream);
rh_status rh_convert_u32_to_f32(float *dst, const uint32_t *src, size_t n, rh_stream stream);
rh_status rh_convert_i64_to_f32(float *dst, const int64_t *src, size_t n, rh_stream stream);
rh_status rh_convert_u64_to_f32(float *dst, const uint64_t *src, size_t n, rh_stream stream);
rh_status rh_convert_f64_to_f32(float *dst, const double *src, size_t n, rh_stream stream);

/* ---- WAV / PCM either side of the path (src/decoder/wav.rs:94-172 ingest, src/wav_output.rs:62-96 egress).
 * probe (host, no GPU): walks the RIFF chunks of a file image.  decode: `data` is a DEVICE copy of the data
 * chunk (8-bit unsigned, 16/24/32-bit signed LE or 32-bit float) AT ANY BYTE ADDRESS -- `file + data_offset` of an uploaded file image
 * is fine: the chunks in front of `data` decide where it starts (the reference's own assets/audacity32bit_int.wav: 32-bit samples at
 * offset 102; tests/wav_test.rs) and hound reads a byte stream; dst receives *out_samples f32 samples --
 * n_samples plus the silence that completes a cut frame (wav.rs:161-169).  header (host): the 44-byte
 * 32-bit-float header wav_to_writer produces, for the whole frames of n_samples (wav_output.rs:98-140);
 * the payload is the f32 block itself.  Returns the bytes written (0 = does not fit). */
typedef struct rh_wav_info {
    uint32_t channels, sample_rate, bits_per_sample;
    int32_t is_float;
    uint64_t data_offset, data_bytes, samples;
} rh_wav_info;
rh_status rh_wav_probe_host(const uint8_t *bytes, size_t size, rh_wav_info *info);
rh_status rh_wav_decode(float *dst, const uint8_t *data, uint64_t n_samples, uint32_t channels,
                        uint32_t bits_per_sample, int32_t is_float, uint64_t *out_samples, rh_stream stream);
/* rh_wav_decode and ChannelCountConverter(channels -> to_channels) (src/conversions/channels.rs:57-85) in ONE pass: what
 * `UniformSourceIterator::new(decoder, to_channels, same rate)` makes of the file (uniform.rs:58-67 -- BASELINE config 5's chain).  dst
 * receives *out_samples = ceil(n_samples / channels) * to_channels samples, bit-identical to rh_wav_decode followed by
 * rh_channels_convert; the decoded block in between (4 bytes a sample written and read again) never exists. */
rh_status rh_wav_decode_channels(float *dst, const uint8_t *data, uint64_t n_samples, uint32_t channels,
                                 uint32_t bits_per_sample, int32_t is_float, uint32_t to_channels,
                                 uint64_t *out_samples, rh_stream stream);
size_t rh_wav_header_f32_host(uint8_t *out, size_t cap, uint32_t channels, uint32_t sample_rate, uint64_t n_samples);

/* ---- ChannelCountConverter: src/conversions/channels.rs:57-85.  Bit-exact.
 * dst holds frames*to_ch samples. */
rh_status rh_channels_convert(float *dst, const float *src, size_t frames, uint32_t from_ch,
                              uint32_t to_ch, rh_stream stream);

/* ---- Amplify: src/source/amplify.rs:64.  dst == src works in place (as for rh_distortion, rh_dither and rh_linear_gain_ramp:
 * a lane reads its four samples before it stores them, and stores no others). */
rh_status rh_amplify(float *dst, const float *src, size_t n, float factor, rh_stream stream);

/* ---- Distortion: src/source/distortion.rs:66-72.  threshold < 0 or NaN: RH_ERR_INVALID (f32::clamp panics). */
rh_status rh_distortion(float *dst, const float *src, size_t n, float gain, float threshold, rh_stream stream);
/* Dither: src/source/dither.rs:217-242.  out = x - noise * lsb with lsb = 1 / 2^(target_bits-1) (:180).
 * algorithm follows the reference's enum order (dither.rs:40-69): 0 GPDF (normal, sigma 0.6), 1 HighPass (blue:
 * white[k] - white[k-channels]), 2 RPDF (uniform [-1,1]), 3 TPDF (triangular (-1,1), the default).
 * The reference seeds a SmallRng from system entropy, so its samples are not reproducible; here the noise of
 * sample k = sample_offset + i is a pure function of (seed, k):
 *   h = mix(seed ^ mix(k + 1)), mix = the splitmix64 finaliser; u1 = (int(h >> 40) - 2^23) / 2^23,
 *   u2 = (int((h >> 16) & 0xffffff) - 2^23) / 2^23; TPDF (u1+u2)/2, RPDF u1, GPDF Box-Muller on the same fields.
 * Stateless: any split of a stream into blocks (with the running sample_offset) equals one pass. */
rh_status rh_dither(float *dst, const float *src, size_t n, uint64_t sample_offset, uint32_t channels,
                    uint32_t target_bits, int32_t algorithm, uint64_t seed, rh_stream stream);
/* ---- LinearGainRamp, fade_in (0 -> 1, then 1.0), fade_out (1 -> 0, clamp_end): src/source/linear_ramp.rs:79-110,
 * fadein.rs:11-13, fadeout.rs:13.  Stateless: sample_offset = samples of the stream already processed. */
rh_status rh_linear_gain_ramp(float *dst, const float *src, size_t n, uint64_t sample_offset, uint32_t channels,
                              uint32_t sample_rate, uint64_t duration_ns, float start_gain, float end_gain,
                              int32_t clamp_end, rh_stream stream);

/* ---- Delay: src/source/delay.rs:8-16,68-75: rh_delay_samples() zeros, then the n input samples (dst holds both).
 * n == 0: src is not read and may be NULL (the same for rh_echo_mix). */
rh_status rh_delay(float *dst, const float *src, uint64_t n, uint64_t delay_samples, rh_stream stream);
/* ---- TakeDuration (+ its fade-out filter): src/source/take.rs:96-148.  src holds n samples of the stream that
 * start at sample_offset; dst (capacity n + channels) receives *out_samples: the samples the duration
 * still admits, then the zeros that complete a cut frame.  *ended = 1 when the duration expires in this
 * block (rodio's None follows).  An upstream that ends first simply stops calling. */
rh_status rh_take_duration(float *dst, const float *src, uint64_t n, uint64_t sample_offset, uint32_t channels,
                           uint32_t sample_rate, uint64_t duration_ns, int32_t fade_out,
                           uint64_t *out_samples, int32_t *ended, rh_stream stream);
/* ... the same from ANY state of the adapter (after `try_seek`, take.rs:222-231: remaining = requested.saturating_sub(pos), the frame
 * position 0): remaining_ns = what is left of the duration at src[0], requested_ns = the adapter's whole duration (the fade-out
 * filter's denominator, :33-38), frame_phase = samples of the current frame already emitted (decides the silence that completes
 * a cut frame, :107-115).  *remaining_after_ns (may be NULL) = what is left behind the samples taken.  Where no sample is
 * taken (n == 0, or remaining_ns below one sample: only the zeros that complete the frame are written) src is not read and may
 * be NULL.  RH_ERR_INVALID: frame_phase >= channels, out_samples == NULL, zero channels or rate. */
rh_status rh_take_duration_from(float *dst, const float *src, uint64_t n, uint64_t remaining_ns, uint64_t requested_ns,
                                uint32_t frame_phase, uint32_t channels, uint32_t sample_rate, int32_t fade_out,
                                uint64_t *out_samples, int32_t *ended, uint64_t *remaining_after_ns, rh_stream stream);

/* ---- ChannelVolume / Spatial: src/source/channel_volume.rs:71-88, src/source/spatial.rs:48-69.
 * gains_host has out_ch entries (out_ch <= 16; more: RH_ERR_UNSUPPORTED).  dst holds frames*out_ch samples; dst == src works
 * in place where in_ch == out_ch. */
rh_status rh_channel_volume(float *dst, const float *src, size_t frames, uint32_t in_ch,
                            const float *gains_host, uint32_t out_ch, rh_stream stream);
/* Host-side: gains[2] from emitter / ear positions (spatial.rs:48-69). */
rh_status rh_spatial_gains(const float emitter[3], const float left_ear[3],
                           const float right_ear[3], float out_gains[2]);

/* ---- Parameters that change while a source plays: PeriodicAccess (src/source/periodic.rs:9-24,63-77) over
 * Amplify::set_factor / set_log_factor (amplify.rs:27-35), ChannelVolume::set_volume (channel_volume.rs:71-88) and
 * Spatial::set_positions (spatial.rs:48-69) -- what Player::append (player.rs:121-166) and SpatialPlayer::append
 * (spatial_player.rs:60-77) wrap every source in.
 * A parameter is a table of STEPS in device memory: sample `first + i` of the stream (counted where the parameter
 * applies) takes entry (first + i) / period - first / period.  Bad arguments (a period of 0, fewer entries than the
 * block reaches, out_ch > 16): RH_ERR_INVALID. */
/* U of PeriodicAccess (periodic.rs:14-22): max(1, (period.as_secs_f32() * rate as f32 * channels as f32) as usize) --
 * SAMPLES, not frames; the closure runs before sample 0, U, 2U, ... of the adapter's stream. */
uint64_t rh_periodic_update_samples(uint64_t period_ns, uint32_t sample_rate, uint32_t channels);
/* Amplify with a factor that changes every `period` samples: dst[i] = src[i] * factors_dev[step(i)] (amplify.rs:64),
 * bit for bit rh_amplify with each step's factor.  Rows start anywhere; dst == src works in place. */
rh_status rh_amplify_steps(float *dst, const float *src, size_t n, uint64_t first, uint64_t period,
                           const float *factors_dev, uint32_t n_factors, rh_stream stream);
/* ChannelVolume with gains that change every `gain_period` OUTPUT samples, optionally followed by Amplify with a
 * factor that changes every `factor_period` (Spatial -> .. -> Amplify, the tail of a SpatialPlayer source, in one launch):
 * out[j] = (m * gains_dev[step_g(j) * out_ch + j % out_ch]) * factors_dev[step_f(j)], m the frame's mean
 * ((0 + s0) + s1 + ..) / in_ch, formed when the output frame begins; each output sample reads the gains of ITS step
 * (channel_volume.rs:71-88: a change in mid-frame reaches the later channels of the frame).  factors_dev may be NULL (no
 * factor).  Bit for bit rh_channel_volume with each step's gains, then rh_amplify_steps.  out_ch <= 16. */
rh_status rh_channel_volume_steps(float *dst, const float *src, size_t frames, uint32_t in_ch, uint32_t out_ch,
                                  uint64_t first, uint64_t gain_period, const float *gains_dev, uint32_t n_gains,
                                  uint64_t factor_first, uint64_t factor_period, const float *factors_dev,
                                  uint32_t n_factors, rh_stream stream);
/* BltFilter whose formula a periodic_access closure changes (blt.rs:68-91, 234-252): coefficients by STEPS, memory kept.
 * Sample i of a stream's block (interleaved, i < frames*channels) is filtered with entry
 * (first + i) / period - first / period of that stream's table; an entry is {b0,b1,b2,a1,a2} as rh_biquad_coeffs gives them.
 * first and period count SAMPLES of the stream, as in rh_amplify_steps: a change reaches channel c with the first sample of that
 * channel at or after the boundary, so it may fall in mid-frame.
 * coeffs_dev: device memory, n_steps entries per stream, table_stride floats between two streams' tables (0: all streams share one).
 * state, n_streams, layout of the batch: as rh_biquad ({x1,x2,y1,y2} per channel; NULL: a zero state that is not kept).  A stream may
 * change between rh_biquad, mode 0 and mode 1 from block to block.  Rows start at any 4-byte address.  frames == 0: nothing happens,
 * state included.  RH_ERR_INVALID: period == 0, channels == 0, fewer entries than the block reaches, 0 < table_stride < 5 * n_steps.
 * No host synchronisation, no allocation per call.
 * mode 0: rodio's operation order (blt.rs:559, left to right, unfused), bit for bit -- rh_biquad mode 0 with each step's entry.  The
 *   drop-in, and the default of the host mirror's live_low_pass / live_high_pass.
 * mode 1: time-parallel.  One workgroup per stream walks the stream's tiles and carries the state itself (no workgroup waits for
 *   another); inside a tile the runs of the lanes are joined by a scan of their affine state maps.  THE CONTRACT: the result is the
 *   f64 evaluation of the same recurrence, every sample rounded to f32 once (within 2^-23 * max(1, peak) of it; the state leaves as
 *   f32).  That is within 1e-5 of rodio's own f32 recurrence for a full-scale source while the table SWEEPS smoothly through filters
 *   that pass rh_filter_scan_ok; it is NOT bounded across jumps between distant filters, where the direct-form state of one filter is
 *   a large transient in the other and rodio's own rounding noise grows with it -- there mode 0 is the drop-in.  f32 recurrence
 *   against the f64 one, full-scale uniform noise at 48 kHz, the table changing every U samples:
 *     low_pass 100 <-> 8000 Hz, geometric sweep, up or down          2.8e-6 / 3.5e-6   (output peak 0.8)
 *     high_pass 600 -> 6000 Hz, geometric sweep                      4.5e-6            (1.45)
 *     stereo U = 441, 6 channels U = 1323, U = 1, q = 2.0            <= 4.6e-6         (up to 2.1)
 *     low_pass ALTERNATING 100 / 8000 Hz every step                  3.8e-4            (12.6)
 *     high_pass alternating 600 / 6000 Hz                            1.25e-5           (4.9)
 *   1 to 8 channels; more channels, and a dst that overlaps src (dst == src is valid), run in mode 0 -- never an error. */
rh_status rh_biquad_steps(float *dst, const float *src, uint64_t frames, uint32_t channels, uint32_t n_streams,
                          uint64_t first, uint64_t period, const float *coeffs_dev, uint32_t n_steps, uint64_t table_stride,
                          float *state, int32_t mode, rh_stream stream);

/* ---- reverb = Mix(x, Delay(Amplify(x))): src/source/mod.rs:628-634, delay.rs:8-16,68-75,
 * mix.rs:43-53.  delay_samples counts INTERLEAVED samples (delay.rs:14).  dst holds
 * n + delay_samples samples. */
uint64_t rh_delay_samples(uint64_t delay_ns, uint32_t sample_rate, uint32_t channels);
rh_status rh_echo_mix(float *dst, const float *src, size_t n, size_t delay_samples, float gain,
                      rh_stream stream);

/* ---- fused, batched reverb -> Spatial (BASELINE config 3): for every stream s < n_streams
 *        Spatial(reverb(x_s, delay, gain), ...) = ChannelVolume(reverb(x_s), gains[s])
 * Replaces source/mod.rs:628-634 + channel_volume.rs:71-88 in one pass over the input.  x_s = src +
 * s*src_stride holds n interleaved STEREO samples; row s of dst (dst + s*dst_stride) receives
 * 2*floor((n + delay_samples)/2) samples.  gains_dev: DEVICE array [n_streams][2] (rh_spatial_gains
 * per stream).  Bit-exact with the two-step reference chain.
 * RH_ERR_INVALID, nothing written: an odd n (the rows are whole stereo frames), dst or src off an 8-byte boundary, an odd dst_stride with
 * more than one stream (every row's output frames are stored as 8-byte pairs).  Rows on 16-byte boundaries with n, delay_samples and both
 * strides multiples of 4 take 16-byte loads and stores; any other shape the 8-byte form -- the same bits. */
rh_status rh_reverb_spatial(float *dst, const float *src, size_t n, size_t delay_samples, float gain,
                            const float *gains_dev, uint32_t n_streams, size_t src_stride,
                            size_t dst_stride, rh_stream stream);

/* ---- SampleRateConverter (+ UniformSourceIterator span chunking):
 * src/conversions/sample_rate.rs:52-90,110-122,131-201, src/math.rs:23-26,
 * src/source/uniform.rs:50-97.  span_len = 0 means current_span_len() == None; otherwise the
 * converter restarts every min(span_len, 32768) SAMPLES like uniform.rs:56.
 * Bit-exact with the reference's lerp (mul, IEEE divide, add; no FMA). */
rh_status rh_resample_out_frames(uint64_t in_frames, uint32_t from_rate, uint32_t to_rate,
                                 uint32_t channels, uint64_t span_len, uint64_t *out_frames);
rh_status rh_resample_linear(float *dst, const float *src, uint64_t in_frames, uint32_t from_rate,
                             uint32_t to_rate, uint32_t channels, uint64_t span_len,
                             rh_stream stream);

/* ---- UniformSourceIterator span by span: src/source/uniform.rs:50-97.  rodio re-builds its converter chain
 *        Take{n: current_span_len().min(32768)} -> SampleRateConverter(from_rate -> to_rate, from_ch) -> ChannelCountConverter(from_ch -> to_ch)
 * whenever the current one runs dry, so a source that reports spans (SamplesBuffer buffer.rs:76-82, Buffered buffered.rs:109,
 * the decoders symphonia.rs:199-201) is converted span by span: each span starts a fresh converter and ends with its last frame
 * verbatim (sample_rate.rs:193-200); rate and layout may change from span to span.  Spans are independent work items, and so
 * are the pieces a span is cut into when it arrives in blocks.  A SEGMENT = output frames [m0, m1) (span-relative) of one span:
 *   src          device pointer to input frame `src_frame0` of the span (src_frames frames of from_ch samples are there)
 *   dst          device pointer: output frame m0 lands at dst[0 .. to_ch)
 *   span_frames  input frames of the WHOLE span once it is complete -- its last frame is then emitted verbatim and nothing
 *                follows; UINT64_MAX while the span is still open (more input will come, or current_span_len() == None)
 * Output frame m reads input frames floor(m*F/T) and +1 (F/T = from/to reduced); the caller keeps the frames the next
 * segment's first tap needs (rh_uniform_first_tap).  Bit-exact with the reference (lerp as mul, IEEE divide, add).
 * A span that ends INSIDE a frame -- uniform.rs:56's `.min(32768)` cuts frames of 3, 5, 6, 7 channels, and a source may return None inside
 * a frame -- is what source/mod.rs:196-200 asks sources not to produce, and rodio plays it anyway: the SampleRateConverter meets a
 * short frame, every output frame that lerps towards it is cut to its length (zip, sample_rate.rs:174-179), the short frame itself
 * comes out verbatim when an output lands on it (:193-200), and the ChannelCountConverter behind regroups those runs into frames of
 * from_ch samples (channels.rs:57-85).  The TAIL of such a span is a segment of its own, marked by reserved = t (the cut frame's
 * samples, 0 < t < from_ch):
 *   span_frames  q, the WHOLE frames of the span
 *   src          device pointer to input frame src_frame0 (= q - src_frames, src_frames in {0, 1}: the frame in front of the cut is
 *                passed whenever an output frame lerps towards the cut frame), followed by the t samples of the cut frame
 *   m0, m1       output SAMPLES [m0, m1) of the tail, 0 <= m0 <= m1 <= rh_uniform_cut_tail_samples(); dst = where sample m0 lands
 * The whole frames in front of the tail convert as the frames of an open span (span_frames = UINT64_MAX: no verbatim last frame).
 * What follows a cut span starts at the sample behind the cut: the caller's stream is a stream of samples, not of frames.
 * rh_uniform_span_frames: output frames computable from the first span_in_frames input frames of a span; complete != 0 adds
 * the verbatim last frame.  rh_uniform_segments validates and launches a host table (any number of segments, sources, formats
 * in one call); the _dev form takes the table from DEVICE memory unvalidated (it can travel in the caller's staging copy);
 * max_out_frames = the largest m1 - m0 in it. */
typedef struct rh_uniform_seg {
    const float *src;
    float *dst;
    uint64_t src_frame0, src_frames;
    uint64_t m0, m1;
    uint64_t span_frames;
    uint32_t from_rate, to_rate;
    uint32_t from_ch, to_ch;
    float gain;          /* Amplify in FRONT of the converter (mixer.add(src.amplify(g)), amplify.rs:64): both taps are scaled
                          * before the lerp, which is the reference's order of operations; 1.0 = none (x * 1.0 == x) */
    uint32_t reserved;   /* 0; t > 0 marks the tail segment of a span that ends t samples into a frame (see above) */
} rh_uniform_seg;
rh_status rh_uniform_span_frames(uint64_t span_in_frames, uint32_t from_rate, uint32_t to_rate, int32_t complete,
                                 uint64_t *out_frames);
rh_status rh_uniform_first_tap(uint64_t out_frame, uint32_t from_rate, uint32_t to_rate, uint64_t *in_frame);
/* Output samples of the tail of a span of span_whole_frames whole frames + tail_samples samples (0 < tail_samples < from_ch). */
rh_status rh_uniform_cut_tail_samples(uint64_t span_whole_frames, uint32_t tail_samples, uint32_t from_rate, uint32_t to_rate,
                                      uint32_t from_ch, uint32_t to_ch, uint64_t *out_samples);
rh_status rh_uniform_segments(const rh_uniform_seg *segs_host, uint32_t n_segs, rh_stream stream);
rh_status rh_uniform_segments_dev(const rh_uniform_seg *segs_dev, uint32_t n_segs, uint64_t max_out_frames,
                                  rh_stream stream);

/* ---- block streaming: the same two adapters when the stream arrives in blocks (what a `Source` shim
 * does: pull a block upstream, process, serve next() from it).  The handle keeps what the reference's
 * iterator keeps between samples; ANY split of a stream into blocks gives the bits of one pass.
 * (rh_biquad / rh_limit / rh_agc carry their state through their `state` argument.)
 *
 * SampleRateConverter, continuous stream (current_span_len() == None; a spanned source is converted span
 * by span with rh_resample_linear, uniform.rs:56-67).  process() consumes in_frames new frames and emits
 * every output frame whose two taps have arrived; flush != 0 marks the end of the stream (rodio's None):
 * the last input frame is then emitted verbatim (sample_rate.rs:193-200).  pending_frames() tells the
 * caller how large dst must be. */
typedef struct rh_resampler rh_resampler;
rh_status rh_resampler_create(rh_resampler **out, uint32_t from_rate, uint32_t to_rate, uint32_t channels);
rh_status rh_resampler_reset(rh_resampler *p);
rh_status rh_resampler_destroy(rh_resampler *p);
rh_status rh_resampler_pending_frames(rh_resampler *p, uint64_t in_frames, int32_t flush, uint64_t *out_frames);
rh_status rh_resampler_process(rh_resampler *p, float *dst, uint64_t dst_capacity_frames, const float *src,
                               uint64_t in_frames, int32_t flush, uint64_t *out_frames, rh_stream stream);
/* reverb (delay_samples interleaved samples, gain): process() maps n samples to n samples; after the last
 * block flush() emits the delay_samples samples of the delayed clone that outlive the source. */
typedef struct rh_echo rh_echo;
rh_status rh_echo_create(rh_echo **out, uint64_t delay_samples, float gain);
rh_status rh_echo_reset(rh_echo *p);
rh_status rh_echo_destroy(rh_echo *p);
rh_status rh_echo_process(rh_echo *p, float *dst, const float *src, uint64_t n, rh_stream stream);
rh_status rh_echo_flush(rh_echo *p, float *dst, rh_stream stream);

/* ---- Mixer: src/mixer.rs:58-66,120-136,175-198.  out[t] = ((0+v0[t])+v1[t])+... over the live
 * sources in insertion order (bit-identical rounding sequence).  Source s contributes samples
 * [start[s], start[s]+len[s]) (start = frame-aligned admission, mixer.rs:175-183).
 * srcs_host / start_host / len_host are host arrays of n_sources entries; dst holds out_len
 * samples = max(start+len).  A source of len 0 is not read and may be NULL; n_sources == 0 writes out_len zeros; a source
 * that runs past out_len is clipped.  The sum is never -0.0 (it starts at +0.0). */
rh_status rh_mix_sum(float *dst, size_t out_len, const float *const *srcs_host,
                     const uint64_t *start_host, const uint64_t *len_host, uint32_t n_sources,
                     rh_stream stream);

/* ---- A block of a mixer of ANY channel count in ONE launch (mixer::mixer(nz!(6), rate): src/mixer.rs:25,185-198), for continuous
 * sources (current_span_len() == None) of any rate and layout: per source Amplify (amplify.rs:64) -> SampleRateConverter
 * (sample_rate.rs:131-201) -> ChannelCountConverter (channels.rs:57-85), i.e. UniformSourceIterator (uniform.rs:58-67), and the
 * ordered sum.  Bit-identical to the chain of stand-alone calls (rh_amplify, rh_resample_linear / rh_uniform_segments,
 * rh_channels_convert, rh_mix_sum) it replaces.  dst receives out_frames frames of `channels` floats: the frames m0 .. m0+out_frames-1
 * of the mix, whatever m0 is -- the caller describes, per source, where those frames lie in what it holds:
 *   data      device pointer to the source frame that holds the FIRST tap of output frame m0: frame floor(m0 F / T) of the source's
 *             stream (F / T = from_rate / to_rate reduced), `channels` interleaved floats a frame
 *   phase     (m0 F) mod T: where frame m0 lies between its taps
 *   frames    output frames of this block the source reaches (<= out_frames): it is silent behind them (it has ended).  Both taps of
 *             every one of them -- frames floor((phase + j F) / T) and the next, counted from data -- must be readable, except
 *   last      ... that a source which has ENDED passes the index (counted from data) of its LAST frame: an output frame whose first
 *             tap is that frame is emitted verbatim (sample_rate.rs:193-200) and its second tap is not read.  Live: UINT32_MAX.
 * 4-byte alignment is all the rows need.  srcs_host is a host array, read before the call returns.  include/rodio_hip.hpp
 * (GpuMixer, mixers of more than two channels) plans the blocks. */
typedef struct rh_wide_src {
    const float *data;
    uint32_t channels, from_rate;
    uint32_t phase;
    uint64_t frames;
    uint32_t last;
    float gain;
} rh_wide_src;
rh_status rh_wide_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                            const rh_wide_src *srcs_host, uint32_t n_sources, rh_stream stream);
/* ... the current block of MANY such mixers in ONE launch: rooms of a voice server, zones of a game world, stems rendered side by side.
 * Mixer b (b < n_mixers) has the destination dsts_host[b] (a device pointer), channels_host[b] channels, the rate to_rates_host[b], a
 * block of out_frames_host[b] frames and src_counts_host[b] sources in insertion order; srcs_host holds the sources of all mixers back to
 * back -- mixer 0's, then mixer 1's, and so on: src_counts_host[0] + .. + src_counts_host[n_mixers - 1] entries, each read exactly as
 * rh_wide_mix_block reads it.  dsts_host[b] receives the bits that
 *     rh_wide_mix_block(dsts_host[b], channels_host[b], to_rates_host[b], out_frames_host[b], <its sources>, src_counts_host[b], stream)
 * writes: the same operations in the same order per output sample.  A mixer with out_frames == 0 is skipped (its dst may be NULL, nothing
 * else of it is looked at); one without sources gets zeros; a source with frames == 0 is not looked at; n_mixers == 0 does nothing.  Rows
 * and destinations need 4-byte alignment only.  The destinations of different mixers must not overlap: the caller's promise, not checked.
 * The six host arrays are read before the call returns.  On `stream`: one copy of the call's tables (from page-locked memory of the
 * library's, into the stream's scratch) and ONE launch, for any number of mixers and any number of sources or rates per mixer; a call
 * whose mixers all have out_frames == 0 queues nothing, and a call of ONE mixer for which rh_wide_mix_block takes one launch (up to 32
 * sources of up to four (rate, phase) pairs, no alike sources of which one ends inside the block) is that launch, without the copy: still
 * one launch a call.  A warmed call neither waits for the stream nor allocates (the first calls on a
 * stream, and a call with larger tables than any before it, do; the fifth call in a row waits until the copy of the first has run).
 * RH_ERR_INVALID, nothing written by any mixer: a NULL array with n_mixers > 0 (srcs_host only where a count is not 0); and of a mixer with
 * out_frames > 0: a NULL dst, channels or to_rate of 0, and what rh_wide_mix_block refuses of a source (frames > 0 with data == NULL, channels
 * or from_rate of 0, frames > out_frames, phase >= T).  RH_ERR_UNSUPPORTED, nothing written: F * T beyond 32 bits; out_frames > 0x7fffffff;
 * a block so long that a source's phase + j F leaves 32 bits, i.e. out_frames > (2^32 - 1 - T) / F -- rh_wide_mix_block cuts such a block
 * into launches, blocks handed over in batches are short; more than 2^31 - 1 tiles of work. */
rh_status rh_wide_mix_batch(float *const *dsts_host, const uint32_t *channels_host, const uint32_t *to_rates_host,
                            const uint64_t *out_frames_host, const uint32_t *src_counts_host, uint32_t n_mixers,
                            const rh_wide_src *srcs_host, rh_stream stream);
/* ... with a low_pass / high_pass on any of its sources: mixer.add(src, gain, filter) of a mixer of more than two channels, a block at a
 * time.  Source s enters the ordered sum as y_s = BltFilter(UniformSourceIterator(Amplify(x_s))) at the mixer's rate and channel count
 * (mixer.rs:58-66, blt.rs:397-492); an unfiltered one as rh_wide_mix_block takes it.  A filtered source that ends inside the block is
 * silent behind its last frame (the filter returns None with its input).  The filters travel as three host arrays parallel to srcs_host
 * (read before the call returns):
 *   kinds_host    -1: no filter, 0: low_pass, 1: high_pass (which side of THE FILTER CONTRACT below the coefficients are held to)
 *   coeffs5_host  5 floats a source, {b0,b1,b2,a1,a2} as rh_biquad_coeffs(kind, freq, q, to_rate) gives them (not read where kind is -1)
 *   states_host   per source a DEVICE pointer to its carried state, 4 * channels floats {x1,x2,y1,y2} per channel (rh_biquad's layout):
 *                 read at the start of the block, written back at its end.  NULL (the entry or the whole array): zero state, not written back.
 * mode as for rh_biquad: 0 = the reference's operation order, bit for bit; 1 = the time-parallel scan (<= 1e-5 for a full-scale source)
 * for the filters inside the contract (rh_filter_scan_ok's rule, applied to the coefficients) and mixes of up to 8 channels, mode 0 for
 * the rest.  On `stream`, in this order: one launch per 32 filtered sources converts them into rows of the mixer's layout (the bits of
 * rh_amplify -> rh_uniform_row) and gathers their states; rh_biquad runs over the rows, ONE call per coefficient set for the rows that
 * span the block (where out_frames * channels is a multiple of 4: the batch form wants rows back to back on 16-byte boundaries; a row
 * each otherwise) and one per row that ends inside it; rh_wide_mix_block sums the original table with every filtered source replaced by
 * its row; one launch per 32 carried states writes them back.  Launches per block therefore grow with the number of coefficient sets,
 * not with the number of filtered sources.  With no filtered source the call IS rh_wide_mix_block.
 * The rows live in `scratch`, a device buffer of the caller's on a 16-byte boundary, at least
 * rh_wide_mix_filtered_scratch_bytes(channels, out_frames, number of filtered sources) bytes -- not in the stream's scratch, which
 * rh_biquad mode 1 claims (and may move) inside the call.  Not needed (NULL) without a filtered source.
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses, kinds_host == NULL, a kind outside -1 .. 1, a filtered source without
 * coefficients, a mode other than 0 / 1, a scratch off its boundary; RH_ERR_CAPACITY: a scratch too small; RH_ERR_UNSUPPORTED: a block
 * so long that a filtered source's position (phase + j F) leaves 32 bits. */
rh_status rh_wide_mix_filtered_scratch_bytes(uint32_t channels, uint64_t out_frames, uint32_t n_filtered, uint64_t *bytes);
rh_status rh_wide_mix_block_filtered(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                                     const rh_wide_src *srcs_host, uint32_t n_sources, const int32_t *kinds_host,
                                     const float *coeffs5_host, float *const *states_host, int32_t mode,
                                     void *scratch, uint64_t scratch_bytes, rh_stream stream);
/* ---- A block of a mixer of SPATIAL EMITTERS in one launch: what SpatialPlayer feeds its mixer (spatial_player.rs:60-77, player.rs:121-166,
 * mixer.rs:58-66).  dst receives out_frames frames of `channels` floats of the mix, in insertion order ((0 + v_0) + v_1) + ..., of
 *     v_s = SampleRateConverter(Amplify(ChannelVolume(x_s)))
 * ChannelVolume (channel_volume.rs:71-88; Spatial is one with two volumes): per source frame the mean ((0 + s0) + s1 + ..) / in_ch, and
 * sample (f, c) of its output is that mean times the gain of channel c, then times the Amplify's factor.  `channels` is the number of
 * volumes AND the mixer's channel count (an emitter with another number of volumes stays a chain of its own).  Gains and factors change
 * by STEPS, by rh_channel_volume_steps' rule: sample (f, c), counted from `data`, has index k = f * channels + c in the adapter's output
 * and takes gain entry (gain_first + k) / gain_period - gain_first / gain_period, column c, and factor entry (factor_first + k) /
 * factor_period - factor_first / factor_period; a change in mid-frame reaches the later channels of that frame, and the two taps of one
 * lerp may lie in different steps.  The converter is rh_wide_mix_block's: i = floor((phase + j F) / T), a + (b - a) * num / T over the
 * scaled samples, the last frame verbatim, F == T passes through.  Bit-identical to rh_channel_volume_steps per source into rows and
 * rh_wide_mix_block over the rows.
 * A source is an rh_wide_src with `channels` = its own channel count (in_ch), data / from_rate / phase / frames / last as
 * rh_wide_mix_block reads them, and gain == 1 (its Amplify is the factor table).  Its tables travel as host arrays parallel to
 * srcs_host, read before the call returns:
 *   gains_dev_host     per source a DEVICE pointer to [entries][channels] floats
 *   gain_steps_host    3 words a source: {gain_first, gain_period, entries}
 *   factors_dev_host   per source a DEVICE pointer to [entries] floats; NULL (the entry or the whole array): no Amplify
 *   factor_steps_host  3 words a source: {factor_first, factor_period, entries} (not read where there are no factors)
 * A table covers the samples of the source frames the block's taps touch, counted from `data`.  Rows and tables need 4-byte alignment
 * only.  A source with frames == 0 is not looked at (data and tables may be NULL).  n_sources == 0 writes zeros.  No host
 * synchronisation, no allocation; launches per block: one per 32 sources, times two where a source ends inside a block of mono sources of
 * one rate into an 8-byte-aligned stereo dst (the frames in front of the end take the kernel that loads a tap once for both ears).
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses of the shared fields, channels == 0 or > 16, an in_ch of 0, a gain other
 * than 1, a period of 0, gains NULL for a source with frames > 0, a table shorter than the block reaches.  A block so long that
 * phase + j F (or a sample index of the step rule) leaves 32 bits is cut into launches. */
rh_status rh_spatial_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                               const rh_wide_src *srcs_host, uint32_t n_sources, const float *const *gains_dev_host,
                               const uint64_t *gain_steps_host, const float *const *factors_dev_host,
                               const uint64_t *factor_steps_host, rh_stream stream);
/* ---- A block of a mixer of PLAYERS in one launch: what Player::append feeds its mixer (player.rs:121-166, mixer.rs:58-66) when the sound
 * it is handed is a fade_in, a fade_out or a linear_gain_ramp.  dst receives out_frames frames of `channels` floats of the mix, in insertion
 * order ((0 + v_0) + v_1) + ..., of
 *     v_s = ChannelCountConverter(SampleRateConverter(Amplify_steps(LinearGainRamp(Amplify_gain(x_s)))))
 * A source is an rh_wide_src read exactly as rh_wide_mix_block reads it (data / channels / from_rate / phase / frames / last; rows need
 * 4-byte alignment only); `gain` is the innermost Amplify, and from_rate is the rate the mixer sees, i.e. behind `speed` (speed.rs relabels
 * it).  Per tap, each a rounded f32 multiply of its own: x * gain, always; * the ramp's factor, where the source has a ramp; * the stepped
 * factor, where it has a table.  Then rh_wide_mix_block's converter -- i = floor((phase + j F) / T), a + (b - a) * num / T with the IEEE
 * division, the last frame verbatim, F == T passes through -- and the channel rule of channels.rs:57-85.  The adapters travel as host
 * arrays parallel to srcs_host, all read before the call returns:
 *   ramps_host         4 words a source: {kind, duration_ns, first_frame, rate}.  kind 0: no ramp, the sample is not multiplied; 1: a
 *                      LinearGainRamp with clamp_end false (fade_in, linear_gain_ramp(.., false)); 2: one with clamp_end true (fade_out).
 *                      rate is the rate the ramp counts time at: the source's own rate IN FRONT OF `speed` (it differs from from_rate
 *                      whenever speed != 1).  first_frame = the frames of the adapter's stream in front of `data`: source frame i,
 *                      counted from data, takes the factor rh_linear_gain_ramp gives frame first_frame + i (linear_ramp.rs:79-110; the same
 *                      for every channel of a frame).  A duration of 0 is a ramp that has run out: 1, or end_gain with clamp_end.
 *                      NULL: no source has a ramp.
 *   ramp_gains_host    2 floats a source: {start_gain, end_gain}; not read where kind is 0; may be NULL where every kind is 0.
 *   factors_dev_host   per source a DEVICE pointer to [entries] floats; NULL (the entry or the whole array): no stepped Amplify
 *   factor_steps_host  3 words a source: {first, period, entries} (not read where there are no factors).  Sample k = f * src_channels + c
 *                      of the source's stream, counted from data, takes entry (first + k) / period - first / period: rh_amplify_steps'
 *                      rule.  A change may fall between the channels of a frame, and the two taps of one lerp may lie in different steps.
 *                      A table covers the samples up to the last one a tap of the block reads.
 * Bit-identical to the chain it replaces: per source rh_amplify -> rh_linear_gain_ramp (sample_offset = first_frame * channels) ->
 * rh_amplify_steps into a row, then rh_wide_mix_block over the rows with gain 1.  A source with frames == 0 is not looked at (its pointers
 * may be NULL); n_sources == 0 writes zeros; out_frames == 0 does nothing.  No host synchronisation, no allocation; one launch per 32
 * sources (earlier where a fifth (rate, phase) pair comes up), later launches continue from the stored partial sum.  A ramp that has run
 * out before the block's first frame costs the kernel one constant.
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses of the shared fields, a kind above 2, a ramp rate of 0 (or beyond 32
 * bits), a ramp without ramp_gains_host, factors without factor_steps_host, a factor period of 0, a factor table shorter than the block's
 * taps reach.  RH_ERR_UNSUPPORTED, nothing written: F * T beyond 32 bits; out_frames > 0x7fffffff; a block so long that a source's
 * phase + j F leaves 32 bits, i.e. out_frames > (2^32 - 1 - T) / F; a source with a factor table of which the block's taps reach more than
 * 2^30 samples.  Such blocks are refused, not cut into launches: blocks are short. */
rh_status rh_player_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                              const rh_wide_src *srcs_host, uint32_t n_sources,
                              const uint64_t *ramps_host, const float *ramp_gains_host,
                              const float *const *factors_dev_host, const uint64_t *factor_steps_host,
                              rh_stream stream);
/* ---- A block of a mixer whose sources may be LOOPS: source.repeat_infinite() (src/source/mod.rs:204, repeat.rs:10-19) handed to Mixer::add
 * or Player::append -- music, ambience, engines --, mixed from ONE resident pass of the sound.  dst receives out_frames frames of `channels`
 * floats of the mix, in insertion order ((0 + v_0) + v_1) + ..., of
 *     v_s = ChannelCountConverter(SampleRateConverter(Amplify(x_s)))
 * A loop is not a modulo on the tap index.  Repeat sits on Buffered (repeat.rs:14), and UniformSourceIterator re-builds its converter chain
 * from what the two report: extract() takes current_span_len().unwrap_or(32768) samples per span (buffered.rs:97-126);
 * Buffered::current_span_len() is the span's WHOLE data.len(), not what is left of it (buffered.rs:207-214); Repeat never returns None, and
 * once `inner` is exhausted it reports the parameters of `next`, the start of the sound (repeat.rs:37-44,58-64); every chain takes
 * current_span_len().min(32768) samples (uniform.rs:56) and starts a fresh SampleRateConverter, whose last frame comes out verbatim
 * (sample_rate.rs:193-200).  Two rules for where the chains cut follow:
 *   rule 0  chains START OVER AT EVERY PASS.  A sound that answers None (decoders, TestSource): Buffered has spans of 32768 samples and a shorter
 *           last one, and every chain is exactly one span; a sound of at most 32768 samples: one span, one chain per pass.  The last frame of
 *           every chain, the pass's last frame included, is verbatim; the next pass starts a new converter at frame 0.
 *   rule 1  chains RUN ON ACROSS THE SEAM.  A SamplesBuffer of more than 32768 samples answers Some(len) (buffer.rs:76-82): Buffered holds ONE
 *           span of the whole sound and always reports len, so every chain is 32768 samples of the UNROLLED stream; the chain grid drifts
 *           against the seam, and a chain that straddles it lerps from the sound's last frame to its first.
 * A source is an rh_wide_src and RH_LOOP_WORDS 64-bit words of loops_host (a host array parallel to srcs_host, read before the call returns):
 *   [0] loop_frames L   the frames of one pass.  0: NOT a loop -- the source is read exactly as rh_wide_mix_block reads it (phase, frames,
 *                       last and all; the other words are ignored), so one music loop and twenty one-shots are one call, the ordered sum intact.
 *   [1] chain_frames c  the input frames a converter chain takes: 1 <= c, c * src.channels <= 32768
 *   [2] rule            0 or 1.  Rule 0: the last chain of a pass takes L mod c frames where that is not 0.  Rule 1 needs L >= c, so a chain
 *                       crosses at most one seam (rodio produces it with L * ch > 32768 >= c * ch only).
 *   [3] chain_start     the source frame (< L) at which the chain in progress at the block's first frame started; rule 0: a multiple of c
 *   [4] chain_out       the output frames of that chain earlier blocks have emitted: less than the chain's output count,
 *                       rh_uniform_span_frames(its input frames, from_rate, to_rate, 1, ..)
 * Of a loop's rh_wide_src: data = frame 0 of the pass (L frames must be readable: every tap is taken inside them); channels, from_rate, gain
 * as rh_wide_mix_block reads them; frames = the block's output frames the loop reaches -- it is silent behind them: a loop the caller stops
 * there; phase and last are not read.  The cursor (words 3 and 4) is small however long the loop has been playing: no position of the
 * kernel depends on the total play time.
 * Bit-identical to the chain it replaces: with the gain in front, under rule 1 rh_uniform_row with span_len = c * channels over an unrolled
 * copy, under rule 0 rh_uniform_row per pass, concatenated; then rh_wide_mix_block over the rows.  The same converter as everywhere: the lerp
 * as mul, IEEE divide, add (math.rs:25), the verbatim last frame, F == T passes through (sample_rate.rs:133-136); channels.rs:57-85 behind
 * it.  Rows need 4-byte alignment only.  A source with frames == 0 is not looked at; n_sources == 0 writes zeros; out_frames == 0 does
 * nothing.  No host synchronisation and no allocation; one launch per 32 sources with frames > 0 (every source carries its own rates: no
 * launch goes early), later launches continue from the stored partial sum.
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses of the shared fields (a loop's phase is not one); loops_host == NULL with
 * n_sources > 0; a rule above 1; c == 0 or c * channels > 32768; rule 1 with L < c; a cursor outside its bounds (chain_start >= L, under
 * rule 0 not a multiple of c, chain_out not below the chain's output count).
 * RH_ERR_UNSUPPORTED, nothing written: F * T beyond 32 bits; out_frames > 0x7fffffff; a source that is not a loop with
 * out_frames > (2^32 - 1 - T) / F (rh_player_mix_block's answer: refused, not cut); and a loop of which a position leaves 32 bits -- with
 * M(n) = rh_uniform_span_frames(n, ..), EXACTLY one of:  L > 2^31;  M(c) * F > 2^32 - 1 (the positions j F of a chain's output frames);
 * under rule 0  P = floor(L / c) * M(c) + M(L mod c) > 2^32 - 1  or  floor(chain_start / c) * M(c) + chain_out + frames - 1 > 2^32 - 1;
 * under rule 1  chain_out + frames - 1 > 2^32 - 1  or  chain_start + floor((chain_out + frames - 1) / M(c)) * c > 2^32 - 1.  (44.1 -> 48 kHz,
 * c = 16384: M(c) F = 2.6e6; no loop of audio rates comes near.)
 *
 * rh_loop_plan: the words of a sound of n_samples samples as rodio would play it, the cursor at 0.  span_len is what the sound handed to
 * repeat_infinite() answers to current_span_len() while fresh: 0 = None -- n_samples <= 32768: c = L, rule 0; otherwise c = 32768 / channels,
 * rule 0.  span_len == n_samples, the SamplesBuffer -- n_samples <= 32768: c = L, rule 0; otherwise c = 32768 / channels, rule 1.  Another
 * constant span_len <= 32768 (decoder packets): c = min(span_len, n_samples) / channels, rule 0.  RH_ERR_UNSUPPORTED for anything that cuts a
 * frame -- n_samples or the chain's samples not a multiple of channels: 3, 5, 6, 7 channels with a sound over 32768 samples; such a loop
 * stays on the unrolled path, as rh_uniform_row plays cut frames -- and for a span_len above 32768 that is not n_samples.  Zero channels or
 * samples, words == NULL: RH_ERR_INVALID.
 * rh_loop_advance: the cursor behind a block of out_frames frames, in place.  ANY cut of a stream into blocks gives the bits of one pass.
 * Words with L == 0 are left as they are.  It refuses what the entry refuses of the words.  Both are host arithmetic: no device, no
 * rh_init needed. */
enum { RH_LOOP_WORDS = 5 };
rh_status rh_loop_plan(uint64_t n_samples, uint32_t channels, uint64_t span_len, uint64_t *words);
rh_status rh_loop_advance(uint64_t *words, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames);
rh_status rh_loop_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                            const rh_wide_src *srcs_host, uint32_t n_sources,
                            const uint64_t *loops_host, rh_stream stream);
/* ---- A block of a mixer whose sources may be QUEUES of sounds played back to back: what Player::append feeds its mixer (src/queue.rs,
 * player.rs:104-108) -- a playlist, a sentence of word samples, an intro and a body --, every sound resident as a whole, each with a channel
 * count, a rate and a gain of its own.  dst receives out_frames frames of `channels` floats of the mix, in insertion order
 * ((0 + v_0) + v_1) + ..., of
 *     v_s = ChannelCountConverter(SampleRateConverter(queue of Amplify(x_k)))
 * THE CHAIN RULE.  A queue is not a concatenation of separately converted sounds.  UniformSourceIterator builds a converter chain from what
 * the queue reports at the moment the previous chain runs dry: it takes current_span_len().min(32768) samples (uniform.rs:56) of channels()
 * at sample_rate() (uniform.rs:58-67); the queue forwards the CURRENT sound's three answers (queue.rs:130-192: the next sound's as soon as
 * the current one is exhausted); a SamplesBuffer answers its WHOLE length, not what is left of it (buffer.rs:76-82); and Take draws its
 * samples from the QUEUE, whatever sounds they come from.  With the STREAM of a queue = the samples of its sounds back to back:
 *   - a chain that starts at stream position p inside sound k takes min(samples_k, 32768) samples of the stream from p on and reads them as
 *     frames of channels_k at rate_k.  A sound of at most 32768 samples that starts on a chain boundary is exactly one chain; a chain that
 *     starts inside a longer sound runs on into the following sounds, reads THEIR samples in sound k's format (a mono sound's samples paired
 *     up as stereo frames) and lerps across the seams.  The next chain starts where it ends, in the format of the sound it starts in.
 *   - a chain ends early only where the sounds run out and the queue has no keep_alive: the queue has ENDED behind it (queue.rs:233-240).
 *   - with keep_alive (every Player's queue) the samples the chain lacks are +0.0 (queue.rs:218-241; no gain multiplies them), the chain goes
 *     on to its full count, and behind it the queue is live and SILENT: it adds +0.0 to every frame it reaches.
 *   - inside a chain of n input frames the converter is the one used everywhere: output frame j (j restarts at 0 with every chain) reads
 *     frames i = floor(j F / T) and i + 1 of the chain, a + (b - a) * num / T with the IEEE division (math.rs:25), the frame with i == n - 1
 *     verbatim (sample_rate.rs:193-200), F == T passes through; n frames give rh_uniform_span_frames(n, from_rate, to_rate, 1, ..) output
 *     frames.  channels.rs:57-85 applies behind it.  Each tap is x * gain of ITS sound, a rounded multiply of its own (amplify.rs:64).
 * A sound is RH_QUEUE_SOUND_WORDS 64-bit words of sounds_host and one float of sound_gains_host (the layout of rh_player_mix_block's ramps: no
 * struct is added): {data, samples, channels, rate} -- data: a device address, `samples` interleaved floats resident as a whole, 4-byte
 * alignment is all it needs, may be 0 where samples == 0 (an empty sound is skipped); channels and rate as the sound reports them (behind
 * `speed`, as rh_player_mix_block words it) -- and gain = the Amplify in FRONT of the queue (sound_gains_host == NULL: every gain is 1).
 * A source is an rh_wide_src, sound_counts_host[s] sounds and RH_QUEUE_WORDS 64-bit words of cursors_host (host arrays, read before the
 * call returns).  sounds_host and sound_gains_host hold the sounds of all sources back to back: source 0's, then source 1's.  A count of 0: NOT a queue -- the
 * source is read exactly as rh_wide_mix_block reads it (phase, frames, last and all; its cursor words are ignored), so one music queue and
 * twenty one-shots are one call, the ordered sum intact.  Of a queue's rh_wide_src only `frames` is read: the block's output frames the
 * queue reaches -- it is silent behind them: a queue the caller stops there; format and gain travel per sound.  A source with frames == 0
 * is not looked at.  The cursor of a queue, small however long it has played:
 *   [0] chain_start  the sample offset into sounds[0] at which the chain in progress at the block's first frame STARTED: the caller lists a
 *                    queue's sounds from that sound on and drops finished ones from the front.  Below sounds[0].samples (0 for an empty one).
 *   [1] chain_out    the output frames of that chain earlier blocks have emitted: less than the chain's output count (at most
 *                    rh_uniform_span_frames(32768 / channels, ..))
 *   [2] state        0 playing, 1 silent (keep_alive, the sounds have run out), 2 ended.  In states 1 and 2 words 0 and 1 are 0, the
 *                    sounds are not looked at and the source adds nothing.  (A count of 0 is a plain source: a queue whose sounds have all
 *                    been dropped is left out of the call, or passed with frames == 0.)
 *   [3] flags        bit 0: keep_alive
 * rh_queue_plan: a fresh queue, the cursor at 0.  rh_queue_advance: the cursor behind a block of out_frames frames, in place, and in
 * *dropped how many sounds the caller drops from the front before the next block (all of them once the state is 1 or 2).  ANY cut of a
 * stream into blocks gives the bits of one pass.  Both are host arithmetic: no device, no rh_init needed.
 * Bit-identical to the chain of entries it replaces: rh_amplify per sound into one concatenated row (zeros behind it for a keep_alive tail),
 * rh_uniform_row per converter chain over its slice with the chain's format, the rows back to back, rh_wide_mix_block over the rows.
 * n_sources == 0 writes zeros; out_frames == 0 does nothing.  On `stream`: one copy of the call's tables (from page-locked memory of the
 * library's into the stream's scratch, as rh_wide_mix_batch does it) and ONE launch for any number of sources, sounds and seams.  A warmed
 * call neither waits for the stream nor allocates (the first calls on a stream, and a call with larger tables than any before it, do; the
 * fifth call in a row waits until the copy of the first has run).
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses of a plain source; dst NULL, channels or to_rate of 0; srcs_host or
 * sound_counts_host NULL with n_sources > 0; sounds_host or cursors_host NULL where a queue reaches a frame; a queue with
 * frames > out_frames; a sound with data 0 and samples > 0, or channels or rate of 0 or beyond 32 bits; a cursor outside its bounds (state > 2, flags > 1,
 * chain_start not below sounds[0].samples unless both are 0, chain_out not below the chain's output count, words 0 / 1 not 0 in state 1 / 2).
 * RH_ERR_UNSUPPORTED, nothing written: out_frames > 0x7fffffff; a plain source with out_frames > (2^32 - 1 - T) / F; and of a chain the
 * block reaches: F * T beyond 32 bits; a sample count that is not a multiple of the chain's channel count (3, 5, 6 or 7 channels with a sound
 * over 32768 samples; a seam chain that ends inside a frame, such as a stereo chain that ends with a mono sound of odd length) -- such a queue
 * stays on the host path (SpanReader in rodio_hip.hpp), as rh_loop_plan words it; M * F > 2^32 - 1 with M the chain's output frames (the
 * kernel computes j F in 32 bits; a chain has at most 32768 samples, so j F < 2^15 T + F: 44.1 -> 48 kHz stereo: 2.6e6).
 * Out of scope: a sound appended to a queue that has already gone idle (queue.rs:136-146: its first frame is a chain of its own, one frame
 * long -- the segment table of rh_queue_mix_plan.h can express it, the planner does not offer it yet); append_with_signal; try_seek;
 * decoders that answer None, or spans shorter than the sound, as the sounds of a queue; GpuMixer planning such blocks in rodio_hip.hpp. */
enum { RH_QUEUE_WORDS = 4, RH_QUEUE_SOUND_WORDS = 4 };
rh_status rh_queue_plan(uint64_t *words, uint32_t keep_alive);
rh_status rh_queue_advance(uint64_t *words, const uint64_t *sounds_host, uint32_t n_sounds,
                           uint32_t to_rate, uint64_t out_frames, uint32_t *dropped);
rh_status rh_queue_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                             const rh_wide_src *srcs_host, uint32_t n_sources,
                             const uint64_t *sounds_host, const float *sound_gains_host,
                             const uint32_t *sound_counts_host, const uint64_t *cursors_host, rh_stream stream);
/* ---- A block of a mixer whose sources may be CLIPS ON A TIMELINE: a resident sound that starts after a delay, is cut to a duration and may
 * fade out over that duration -- what sequencers, samplers, game schedulers and the "a" side of a crossfade add to a mixer:
 *     mixer.add(sound.amplify(g).take_duration(len) [.set_filter_fadeout()] .delay(at))        (skip_duration(d) in front: the in-point)
 * dst receives out_frames frames of `channels` floats of the mix, in insertion order ((0 + v_0) + v_1) + ..., of
 *     v_s = ChannelCountConverter(SampleRateConverter(stream of the clip))
 * THE STREAM.  With x a sound of n interleaved samples of ch channels at rate fr, all integers exact:
 *   Z   = floor(delay_ns * ch * fr / 10^9) samples of +0.0 come first (delay.rs:8-16,68-75); Z need not be a multiple of ch.
 *   dps = floor(10^9 / (fr * ch)) ns a sample; N = min(n, floor(take_ns / dps)) samples are admitted (take.rs:107-147); without a take N = n.
 *   With the fade-out filter admitted sample k (counted over all channels) is (x_k * g) * R / Tt, R = float(floor((take_ns - k dps) / 10^6)),
 *   Tt = float(floor(take_ns / 10^6)): two roundings, steps of one millisecond (take.rs:33-41); take_ns < 1 ms gives x * 0 / 0, as
 *   rh_take_duration and rh_crossfade have it.  x_k * g is a rounded multiply of its own (amplify.rs:64); the zeros are not multiplied.
 *   The stream is those Z + N samples, read as frames of ch samples BY STREAM POSITION: with Z mod ch != 0 a frame pairs samples across
 *   the sound's own frames, from the first frame on, which straddles the zeros and the sound.
 * THE CHAIN RULE.  UniformSourceIterator takes current_span_len().min(32768) samples per converter chain (uniform.rs:56); Delay adds its
 * remaining zeros to the inner answer (delay.rs:94-98); TakeDuration ALWAYS answers Some(min(inner, remaining)) (take.rs:180-196); a
 * SamplesBuffer answers its whole length (buffer.rs:76-82).
 *   rule G  with a take, or a sound that answers Some(whole length): chains cut the stream at every multiple of 32768 samples from stream
 *           position 0 -- the leading zeros are lerped into the sound's first frame, a grid line inside the sound ends a chain with a
 *           verbatim frame --, the last chain takes what is left.
 *   rule C  no take and a sound that answers None: the stream is one chain.
 * Inside a chain of f frames the converter is the one used everywhere: output frame j reads frames i = floor(j F / T) and i + 1 of the
 * chain, a + (b - a) * num / T with the IEEE division (math.rs:25), the frame with i == f - 1 verbatim (sample_rate.rs:193-200), F == T
 * passes through; f frames give rh_uniform_span_frames(f, from_rate, to_rate, 1, ..) output frames; channels.rs:57-85 applies behind it.
 * Behind its last chain the clip has ended.  (Where the duration expires inside a frame TakeDuration completes the frame with silence,
 * take.rs:109-123; the last chain has taken its Z + N samples by then and that silence is never drawn.)
 * A source is an rh_wide_src and RH_CLIP_WORDS 64-bit words of clips_host (a host array parallel to srcs_host, read before the call returns):
 *   [0] kind      0: NOT a clip -- the source is read exactly as rh_wide_mix_block reads it (phase, frames, last and all; the other words are
 *                 ignored), so scheduled clips and plain sources are one call, the ordered sum intact.  1: rule G.  2: rule C.
 *   [1] Z   [2] N   [3] take_ns (0 without a take)   [4] flags: bit 0 a take is present, bit 1 the fade-out filter is set
 *   [5] done      THE CURSOR: output frames of the clip that earlier blocks have emitted.  It is all the state there is: the chain in
 *                 progress and the frame inside it (rule G), the first tap and its phase (rule C) follow from it on the host, in exact
 *                 integer arithmetic, and the kernel sees positions counted from that chain's first sample only -- no position of the
 *                 kernel depends on Z or on how long the clip has played.
 *   [6] total     output frames of the whole clip at the rates of the last rh_clip_advance: `done == total` is the end.  rh_clip_plan does
 *                 not know the mixer's rate and leaves 0; rh_clip_advance(words, .., 0) behind the plan states it.  The entry does not
 *                 read this word (it works the count out itself).
 * Of a clip's rh_wide_src: data = sample 0 of the sound, BEHIND the in-point (skip_duration(d) skips floor(d * fr / 10^9) * ch samples,
 * skip.rs:62-71: the caller's offset into its buffer; a skipped SamplesBuffer goes on answering Some), N samples must be readable;
 * channels, from_rate and gain as everywhere; frames = the block's output frames the clip reaches, at most total - done (frames of the
 * delay count: they are frames of the clip); phase and last are not read.  A source with frames == 0 is not looked at.
 * Bit-identical to the chain it replaces -- rh_amplify -> rh_take_duration (fade_out) -> rh_delay into one row of Z + N samples,
 * rh_uniform_row over the row with span_len = the row's length under rule G and 0 under rule C, rh_wide_mix_block over the rows with gain
 * 1 -- and to the reference's Mixer fed the adapter chains.  Rows need 4-byte alignment only.  n_sources == 0 writes zeros; out_frames == 0
 * does nothing.  On `stream`: the table travels by value, 32 sources with frames > 0 a launch, later launches continue from the stored
 * partial sum; the number of launches depends on the number of sources only, never on delays, takes or grid lines crossed.  No host
 * synchronisation and no allocation.
 * RH_ERR_INVALID, nothing written: what rh_wide_mix_block refuses of the shared fields (a clip's phase is not one); dst NULL, channels or
 * to_rate of 0; srcs_host or clips_host NULL with n_sources > 0; words out of bounds: kind > 2, flags > 3, the fade-out without a take, rule C
 * with a take, N above floor(take_ns / dps) with a take, done > total, a clip with frames > total - done.
 * RH_ERR_UNSUPPORTED, nothing written: a chain that would end inside a frame -- (Z + N) mod ch != 0, or under rule G Z + N > 32768 with
 * 32768 mod ch != 0 (3, 5, 6, 7 channels): such a clip stays on the row path, as rh_loop_plan words it; F * T beyond 32 bits;
 * out_frames > 0x7fffffff; a plain source with out_frames > (2^32 - 1 - T) / F; Z, N or Z + N above 2^62, a total above 2^63, dps == 0 with a
 * take (fr * ch > 10^9: rh_take_duration's answer); and what leaves 32 bits within ONE block -- with c = 32768 / ch where Z + N > 32768 under
 * rule G and (Z + N) / ch otherwise, M = rh_uniform_span_frames(c, ..), EXACTLY one of:
 *   rule G   M * F > 2^32 - 1;  j0 + frames - 1 > 2^32 - 1 with j0 = done mod M;
 *            min((floor((j0 + frames - 1) / M) + 1) * c * ch, Z + N - floor(done / M) * c * ch) > 2^32 - 1   (the samples the block's chains span)
 *   rule C   r0 + (frames - 1) * F > 2^32 - 1 with r0 = (done * F) mod T;
 *            min((floor((r0 + (frames - 1) * F) / T) + 2) * ch, Z + N - floor(done * F / T) * ch) > 2^32 - 1
 * A plain source is bounded as rh_wide_mix_block bounds it, by its positions phase + j F alone: its sample indices frame * channels may
 * pass 2^32 (8 channels with F == T beyond 2^29 frames) and are formed in 64 bits, as that entry forms them.
 * (44.1 -> 48 kHz stereo: M F = 2.6e6, and a block of 2^31 - 1 frames spans 3.9e9 samples: no block of audio comes near.)  The fade's
 * millisecond index is 32-bit arithmetic per tap where (those samples) * dps + 999999 and the remaining milliseconds at the block's first
 * chain fit 32 bits -- every block below 10^5 frames at audio rates --, 64-bit otherwise: slower, the same bits, never refused.
 * rh_clip_plan: the words of a sound of n_samples samples behind the in-point, the cursor at 0.  span_len is what the sound answers to
 * current_span_len(): 0 = None, a value >= n_samples = its whole length; anything between is RH_ERR_UNSUPPORTED (decoder packets cut
 * chains elsewhere), and so is a clip that cuts a frame (above).  flags above 3, the fade-out without a take, zero channels or rate, words
 * == NULL: RH_ERR_INVALID.  rh_clip_advance: the cursor behind a block of out_frames frames, in place (it stops at `total`), and word 6;
 * `channels` and from_rate are the sound's.  ANY cut of a stream into blocks gives the bits of one pass.  Words of kind 0 are left as they
 * are.  It refuses what the entry refuses of the words.  Both are host arithmetic: no device, no rh_init needed.
 * Out of scope: GpuMixer planning such blocks in rodio_hip.hpp; constant decoder spans shorter than the sound; clips that cut a frame;
 * fade_in, ramps and stepped volume on a clip (rh_player_mix_block has them); try_seek; loops or queues as clips. */
enum { RH_CLIP_WORDS = 7 };
rh_status rh_clip_plan(uint64_t *words, uint64_t n_samples, uint32_t channels, uint32_t rate, uint64_t span_len,
                       uint64_t delay_ns, uint64_t take_ns, uint32_t flags);
rh_status rh_clip_advance(uint64_t *words, uint32_t channels, uint32_t from_rate, uint32_t to_rate, uint64_t out_frames);
rh_status rh_clip_mix_block(float *dst, uint32_t channels, uint32_t to_rate, uint64_t out_frames,
                            const rh_wide_src *srcs_host, uint32_t n_sources,
                            const uint64_t *clips_host, rh_stream stream);

/* ---- Mix, the two-input combinator: Source::mix(other) (src/source/mod.rs:255, src/source/mix.rs:10-22).  Mix::next (mix.rs:43-53) over two
 * rows that are already in the mix's format: dst[i] = a[i] + b[i] for i < min(na, nb) -- s1 + s2 with no leading zero, so -0.0 + -0.0 stays
 * -0.0 (rh_mix_sum is the MIXER's ((0 + v0) + v1)) -- and where one side has ended the other side's samples follow VERBATIM, bit for bit
 * (mix.rs:47-52: not s + 0.0).  dst holds max(na, nb) samples.  Rows start at any 4-byte-aligned address; dst == a and dst == b work in
 * place; na == 0, nb == 0 and both are legal. */
rh_status rh_mix_pair(float *dst, const float *a, size_t na, const float *b, size_t nb, rh_stream stream);
/* ---- UniformSourceIterator::new(src, to_ch, to_rate) over a row that is resident as a whole: src/source/uniform.rs:50-97 -- what Mix::new wraps
 * its second input in (mix.rs:14-21; the first input's wrapper is the identity on samples).  span_len as rh_resample_linear (0 = None):
 * every min(span_len, 32768) SAMPLES a fresh converter chain whose last frame comes out verbatim, the last chain over what is left.  A
 * chain that ends inside a frame (spans of 1000 samples of a 6-channel source; a row that ends in mid-frame) is converted as rodio plays
 * it (the tail segment of rh_uniform_seg) and the next chain starts behind the cut; rh_resample_linear refuses those.  The segments go
 * through rh_uniform_segments.  dst_capacity below rh_uniform_row_out_samples(): RH_ERR_INVALID, nothing written. */
rh_status rh_uniform_row_out_samples(uint64_t n_samples, uint32_t from_ch, uint32_t from_rate, uint32_t to_ch, uint32_t to_rate,
                                     uint64_t span_len, uint64_t *out_samples);
rh_status rh_uniform_row(float *dst, uint64_t dst_capacity, const float *src, uint64_t n_samples, uint32_t from_ch, uint32_t from_rate,
                         uint32_t to_ch, uint32_t to_rate, uint64_t span_len, uint64_t *out_samples, rh_stream stream);
/* ---- Source::take_crossfade_with(other, duration) (src/source/mod.rs:448, src/source/crossfade.rs:10-23), fused and batched:
 *        Mix(a.take_duration(d) with set_filter_fadeout(), b.take_duration(d).fade_in(d))
 * for n_pairs pairs in ONE launch.  `a` starts at the sample where the crossfade begins and sets the output's format; its sample o is
 * multiplied by remaining.as_millis() as f32 and divided by total.as_millis() as f32 (take.rs:33-41: a duration under 1 ms gives
 * x * 0 / 0).  `b` is in its own format: TakeDuration (take.rs:96-148), the fade-in ramp at b's own rate (linear_ramp.rs:79-110,
 * fadein.rs:11-13), then UniformSourceIterator (uniform.rs:50-97) in chains of min(span, 32768) samples, span = what the duration admits
 * unless b_span_len (0 = None) is shorter (take.rs:180-196, linear_ramp.rs:121-123) -- every chain a fresh converter (math.rs:23-26,
 * sample_rate.rs:131-201) whose last frame is verbatim, then channels.rs:57-85 -- and the four arms of mix.rs:43-53.  A duration that
 * expires inside a frame of b ends b's chain in front of the silence that completes the frame (take.rs:109-123), so the output may end
 * inside a frame.  dst receives rh_crossfade_out_samples() samples (written to out_samples_host[pair] unless that is NULL).
 * The fused kernel takes b of 1 or 2 channels, a of up to 8, any two rates, admitted sample counts that are whole frames on both sides
 * and chains of whole frames; any other pair (a cut frame, a 6-channel b, a span that cuts frames) runs through rh_take_duration,
 * rh_linear_gain_ramp, rh_uniform_row and rh_mix_pair on the stream's scratch: never an error, the same bits, slower.  Zero channels or
 * rate, or a capacity below rh_crossfade_out_samples(): RH_ERR_INVALID, and no pair of the batch is written. */
/* A pair travels as RH_CROSSFADE_PAIR_WORDS 64-bit words (a host table, read before the call returns), in this order:
 *   [0] a: device address of the row in the output's format   [1] a_samples   [2] a_channels   [3] a_rate
 *   [4] b: device address of the row in its own format         [5] b_samples   [6] b_channels   [7] b_rate
 *   [8] b_span_len: current_span_len() of b, 0 = None          [9] dst: device address         [10] dst_capacity, in samples */
enum { RH_CROSSFADE_PAIR_WORDS = 11 };
/* rh_crossfade stages its table in a ring of four page-locked slots per stream: of calls queued back to back on a stream that is
 * backed up, the fifth waits until the copy of the first has run. */
rh_status rh_crossfade_out_samples(const uint64_t *pair_host, uint64_t duration_ns, uint64_t *out_samples);
rh_status rh_crossfade(const uint64_t *pairs_host, uint32_t n_pairs, uint64_t duration_ns, uint64_t *out_samples_host,
                       rh_stream stream);

/* ---- BltFilter (low_pass / high_pass): src/source/blt.rs:502-544,558-560,397-492.
 * kind: 0 = low_pass, 1 = high_pass.  coeffs5 = {b0,b1,b2,a1,a2} (already divided by a0).
 * state (optional device pointer, 4*channels floats {x1,x2,y1,y2} per channel) carries the
 * filter across blocks; NULL = zero state, not written back.
 * mode 0 = sequential per (source,channel) stream, same op order as blt.rs:559 (bit-exact);
 * mode 1 = time-parallel scan (<=1e-5 abs): 1 to 8 channels, the same state as mode 0 (a stream may
 *          change modes between blocks).  A call the scan kernel does not take -- rows that do not start on 16-byte boundaries
 *          (dst, src, and frames*channels % 4 == 0 for n_streams > 1), more than 8 channels, a filter that does not forget
 *          within 64 tiles, dst == src (the scan reads the two frames in front of every share after a neighbour may have
 *          overwritten them) -- runs in mode 0 instead: never an error, the exact bits, slower.
 * The batch form filters n_streams equally shaped blocks laid out back to back.  Mode 0 works in place.
 * Mode 1 keeps the device tables of its 32 most recent filters; a call with a 33rd frees the oldest, and that free may wait for the
 * device. */
rh_status rh_biquad_coeffs(int32_t kind, uint32_t freq, float q, uint32_t sample_rate,
                           float out_coeffs5[5]);
rh_status rh_biquad(float *dst, const float *src, uint64_t frames, uint32_t channels,
                    uint32_t n_streams, const float coeffs5_host[5], float *state, int32_t mode,
                    rh_stream stream);
/* THE FILTER CONTRACT.  Every time-parallel evaluation of a low_pass / high_pass in this library (rh_biquad mode 1, the fused rh_rlm_*
 * path, its streamed blocks) is held to two things, on noise, DC, steps, impulses, tones at the cutoff, a Nyquist alternation and tails
 * that fall silent, through real, double and complex poles (tests/test_gpu_filter_signals.py, profiles/filter_signals.txt):
 *   (B) it is no further from the exact (f64) response than rodio's own f32 recurrence: |scan - exact| <= 2 |rodio - exact| + F, where
 *       F = 8 * 2^-24 * max|x| * sum|h| is a handful of f32 roundings at the size of the terms a time-parallel evaluation adds up;
 *   (C) it is within 1e-5 * peak of rodio's samples (peak = max(1, max|y|)) wherever rodio itself is within 5e-6 * peak of the exact
 *       response.
 * Where rodio is further from the exact response than that, |scan - rodio| IS rodio's rounding noise, which the recurrence amplifies by
 * ~1 / (1 - r)^2 for poles of radius r.  rh_filter_scan_ok returns 1 where that noise stays <= 1e-5 for full-scale WHITE NOISE
 * (|x| <= 1; it scales with the peak): low_pass with 1 - r >= 0.0125 (>= 100 Hz at 48 kHz), high_pass with 1 - r >= 0.075 (>= 600 Hz
 * at 48 kHz); measured table: profiles/r04_filter_contract.txt.  On DC-heavy material through a low cutoff rodio's recurrence is biased
 * by more than that although the filter passes: |rodio - exact| at 48 kHz, one channel, 24 000 frames --
 *       filter                    noise      DC 1.0     tone at the cutoff
 *       low_pass  100, q 0.5      6.3e-6     3.1e-4     1.8e-5
 *       low_pass  200, q 0.5      2.1e-6     6.5e-5     6.3e-6
 *       low_pass  300, q 0.35     9.8e-7     1.1e-5     3.2e-6
 *       low_pass  800, q 2.0      2.7e-6     8.4e-6     8.2e-6   (peak 2.0)
 *       low_pass 1000, q 0.5      6.2e-7     4.0e-6     5.2e-7
 *       low_pass 1000, q 0.7071   1.2e-6     2.0e-6     9.7e-7
 * -- while the scan stays within 1.1e-6 of the exact response on the rows from 200 Hz up (measured on an MI355X), so on such material it differs
 * from rodio by rodio's bias: (C) does not apply there, (B) does.  0 outside the thresholds: a drop-in for rodio's samples then takes
 * rh_biquad mode 0 (the reference's order, bit for bit) -- include/rodio_hip.hpp does so on its own (GpuSource: per filter; GpuMixer:
 * the source gets a chain amplify -> uniform -> filter in mode 0 of its own and enters the mixer unfiltered); a caller that needs
 * rodio's samples on DC through a low cutoff asks for mode 0 itself (exact_filters(true)). */
int32_t rh_filter_scan_ok(int32_t kind, uint32_t freq, float q, uint32_t sample_rate);

/* ---- src/math.rs:51-56,86-90,110-113 (host): dB <-> linear as the reference spells them (2^(dB*0.05*log2 10),
 * log2(x)*log10(2)*20) and the smoothing coefficient exp(-1/(seconds*rate)) of the limiter and the AGC.
 * Amplify::set_log_factor / Source::amplify_decibel (amplify.rs:33-35) is rh_amplify with rh_db_to_linear(dB). */
float rh_db_to_linear(float decibels);
float rh_linear_to_db(float linear);
float rh_duration_to_coefficient(uint64_t duration_ns, uint32_t sample_rate);

/* ---- Limit: src/source/limit.rs:94-130,853-988.  state: 2*channels floats
 * {integrator, peak} per channel (optional).  Works in place (dst == src).  A hand-off that expires inside the
 * kernel poisons the output with NaN and is reported by rh_async_status().
 * Parity is by TOLERANCE only (<= 1e-5 abs, tested): the time-parallel kernel evaluates log2 / exp2 with the device's instructions, composes the
 * integrator and peak recurrences as max-affine maps and, inside a run, spells them mul + FMA where limit.rs:909-913 has mul, mul, add (one
 * rounding fewer per step).  RH_LIMIT_SEQ=1 takes the one-lane-per-stream kernel in the reference's operation order throughout. */
typedef struct rh_limit_params {
    float threshold_db; /* LimitSettings::threshold  (default -1) */
    float knee_width_db;/* LimitSettings::knee_width (default 4)  */
    uint64_t attack_ns; /* default 5 ms   */
    uint64_t release_ns;/* default 100 ms */
} rh_limit_params;
rh_status rh_limit(float *dst, const float *src, uint64_t frames, uint32_t channels,
                   uint32_t sample_rate, uint32_t n_streams, const rh_limit_params *params_host,
                   float *state, rh_stream stream);

/* ---- AutomaticGainControl: src/source/agc.rs:133-171,397-504.  One state for all interleaved
 * channels of a stream.  state (optional): rh_agc_state_floats() floats per stream.
 * NaN / Inf input: as the reference (agc.rs:150,406,422-426,453-457, derived in tests/golden/derive_traces.py): the sample comes out NaN, the
 * window sum and the peak level stay NaN, both `> 0.0` tests fail from then on and the gain climbs to absolute_max_gain and stays there. */
typedef struct rh_agc_params {
    float target_level;      /* default 1.0 */
    uint64_t attack_ns;      /* default 4 s; clamped to 10 s like source/mod.rs:432-433 */
    uint64_t release_ns;     /* default 0 */
    float absolute_max_gain; /* default 7.0 */
    float floor;             /* default 0.0 */
} rh_agc_params;
size_t rh_agc_state_floats(void);
/* Resets n_streams states to a fresh AGC (gain 1.0, empty RMS window): agc.rs:209-236. */
rh_status rh_agc_state_init(float *state, uint32_t n_streams, rh_stream stream);
rh_status rh_agc(float *dst, const float *src, uint64_t n_samples, uint32_t sample_rate,
                 uint32_t n_streams, const rh_agc_params *params_host, float *state,
                 rh_stream stream);

/* ---- fused pipeline (BASELINE config 2): for every source
 *        mixer.add(UniformSourceIterator::new(src, ch, to_rate).low_pass(freq))
 *      then the ordered mixer sum -- one kernel, each input byte read once.
 * Replaces uniform.rs:78-97 + sample_rate.rs:131-201 + blt.rs:397-451 + mixer.rs:185-198. */
typedef struct rh_rlm_config {
    uint32_t from_rate, to_rate;
    uint32_t channels;     /* 1 (mono) or 2 (stereo): the frames of every source and of the mix (other layouts: rh_channels_convert / rh_uniform_segments in front) */
    uint64_t span_len;     /* 0 = None; else chunk of min(span_len, 32768) samples */
    int32_t filter_kind;   /* 0 = low_pass, 1 = high_pass, -1 = no filter, 2 = custom_coeffs; from_rate == to_rate: the converter passes through */
    uint32_t filter_freq;
    float filter_q;        /* rodio's low_pass() uses 0.5 (blt.rs:11-16) */
    uint32_t max_sources;
    uint64_t max_in_frames;
    uint32_t frames_per_lane; /* output frames per lane of a 64-lane tile; 0 = auto */
    uint32_t ring_stages;     /* LDS stages of the source prefetch ring (2..4); 0 = auto */
    uint32_t no_balance;      /* diagnostics: 1 = do not pad the LDS request to even out waves per CU */
    uint32_t force_general;   /* diagnostics/tests: 1 = use the ragged-batch kernel even for equal lengths */
    float custom_coeffs[5];   /* filter_kind 2: {b0,b1,b2,a1,a2}, already divided by a0 */
    uint32_t filter_first;    /* 1 = `mixer.add(src.low_pass(f))`: the filter runs on every source BEFORE the converter, at from_rate (source/mod.rs:255-275:
                               * a filter takes its sample rate from its input; mixer.rs:58-66 converts what it is given).  0 = the benchmark's spelling,
                               * `mixer.add(UniformSourceIterator::new(src, ..).low_pass(f))`: convert, then filter at to_rate.  With 1, one-shot runs of
                               * equal-length batches (sum the sources, filter that one stream, convert it: three linear stages, compared at 1e-5);
                               * rh_rlm_run on sources of different lengths and the rh_rlm_stream_* calls return RH_ERR_UNSUPPORTED. */
} rh_rlm_config;
typedef struct rh_rlm rh_rlm;
rh_status rh_rlm_create(rh_rlm **out, const rh_rlm_config *cfg);
rh_status rh_rlm_destroy(rh_rlm *p);
/* srcs_host[s] = device pointer of source s ([in_frames_host[s]][channels] f32, 16-byte
 * aligned).  All sources start at mixer time 0.  dst holds out_capacity_frames*channels
 * samples; *out_frames = max over sources of the resampled length.
 * On a handle that has run, rh_rlm_set_sources and rh_rlm_set_sources_pcm16 wait until everything the handle has queued on its stream has completed. */
rh_status rh_rlm_set_sources(rh_rlm *p, const float *const *srcs_host,
                             const uint64_t *in_frames_host, uint32_t n_sources);
/* srcs_host[s] = device pointer of source s as interleaved signed 16-bit PCM ([in_frames_host[s]][channels] int16_t, the layout of a
 * WAV data chunk).  Equivalent, bit for bit, to rh_convert_i16_to_f32 of every row followed by rh_rlm_set_sources (dasp's i16 -> f32,
 * `s as f32 / 32768.0`, is exact).  The arguments follow rh_rlm_set_sources' rules, except that a row may start on any 2-byte boundary;
 * either entry replaces what the other set; rh_rlm_set_gains and rh_rlm_set_filters work unchanged.  The sources serve the one-shot
 * entries (rh_rlm_run, _run_subset, _run_batch, _autotune); the stream entries take f32 rows per block as before.
 * NATIVE runs -- the kernels read the int16 rows themselves, no decoded copy exists -- are the whole one-shot runs (rh_rlm_run) of a
 * filtered batch of equal lengths on a handle without filter_first and without rh_rlm_set_filters:
 *   - rh_rlm_geometry_info::mix_first == 2 (k_rlm_chunk_pcm16): every row on a 16-byte boundary and a whole number of 16-byte vectors
 *     (frames * channels % 8 == 0);
 *   - mix_first == 1 where the rows are summed by k_mix_rows (k_mix_rows_pcm16; not k_mix_ring): every row on an 8-byte boundary, any length.
 * Every other run -- no filter, different lengths, force_general, filter_first, rh_rlm_run_subset, rh_rlm_run_batch, per-source filters,
 * k_mix_ring's rows, rows off those boundaries -- reads an f32 copy of the rows, which the first such run makes on its stream
 * (rh_convert_i16_to_f32) ONCE per rh_rlm_set_sources_pcm16 and which goes when the sources are replaced or the handle is destroyed:
 * never an error, the same bits.  RH_ERR_NOMEM (from that run; from this call on a handle with per-source filters): no memory for the copy.
 * A stream that runs on the handle afterwards puts its own blocks in the sources' place: a one-shot run behind it returns RH_ERR_INVALID until
 * the sources are set again. */
rh_status rh_rlm_set_sources_pcm16(rh_rlm *p, const int16_t *const *srcs_host, const uint64_t *in_frames_host, uint32_t n_sources);
/* *format: 0 = the sources set are f32 rows, 1 = PCM16 rows.  *native: 1 = the last one-shot run read the PCM16 rows themselves,
 * 0 = it ran on f32 rows (f32 sources, or a converted copy of PCM16 ones). */
rh_status rh_rlm_source_format(rh_rlm *p, int32_t *format, int32_t *native);
/* Optional per-source Amplify factors (src/source/amplify.rs:64; Player::set_volume): source s contributes
 * gains[s] * (its converted, filtered stream).  The chain is linear, so it does not matter where in it rodio
 * applies the factor; without a filter the result stays bit-identical to amplify-then-convert.  Sources beyond
 * n keep 1.0.  Takes effect for the sources that are set and for every later set_sources / stream block. */
rh_status rh_rlm_set_gains(rh_rlm *p, const float *gains_host, uint32_t n);
/* A filter PER SOURCE: `mixer.add(a.low_pass(200)); mixer.add(b.high_pass(300)); mixer.add(c)` -- in rodio every source carries its own
 * adapters into Mixer::add (src/source/mod.rs:686-721, src/mixer.rs:58-66).  kinds/freqs/qs are host arrays of n entries (kind as
 * rh_rlm_config.filter_kind: -1 none, 0 low_pass, 1 high_pass; q 0.5 is rodio's low_pass()/high_pass()); sources beyond n keep the
 * handle's own filter; n == 0 returns to it for all.  Sources with the same (kind, freq, q) form a class; every class runs as a fused
 * launch of its own -- summed at the input rate first where its sources share a length, the bit-exact ordered sum
 * where it has no filter -- and the classes' mixes are added in order of first appearance (f32; <= 1e-5 from rodio's per-sample order
 * like every filtered path).  Call before rh_rlm_set_sources (which deals the sources over the classes); rh_rlm_set_gains may follow
 * either.  One-shot runs (rh_rlm_run, rh_rlm_autotune); rh_rlm_run_subset / _batch and the stream entries return RH_ERR_UNSUPPORTED on
 * such a handle (a streaming host keeps one handle per filter: include/rodio_hip.hpp GpuMixer::add(src, gain, filter)). */
rh_status rh_rlm_set_filters(rh_rlm *p, const int32_t *kinds_host, const uint32_t *freqs_host, const float *qs_host, uint32_t n);
/* May the launches of this handle assume that they have the device to themselves?  exclusive != 0 (the default: a one-shot job on
 * its own): a launch whose tiles are all resident at once numbers them by workgroup index.  exclusive == 0: other work shares the
 * CUs while the handle runs -- a collective on a second stream (the N > 1 ranks of bench.py: the all-reduce of block k overlaps the
 * kernel of block k+1), copy launches (GpuMixer), another process -- and tiles are handed out by ticket, which needs neither full
 * residency nor in-order dispatch: a tile only ever waits for tiles that already hold a wave slot.  Same results either way. */
rh_status rh_rlm_set_exclusive(rh_rlm *p, int32_t exclusive);
/* "Mix first" (DESIGN.md 4.6): filtered sources of one length and one filter are summed at the input rate and converted and
 * filtered once (the converter and the filter are linear).  enable == 0 keeps every source on its own through the converter and
 * the filter (what a batch of per-source filters or lengths takes anyway); results agree within the 1e-5 of the filtered path.
 * Takes effect from the next run / stream block. */
rh_status rh_rlm_set_mix_first(rh_rlm *p, int32_t enable);
rh_status rh_rlm_run(rh_rlm *p, float *dst, uint64_t out_capacity_frames, uint64_t *out_frames,
                     rh_stream stream);
/* The same over the sources [first, first+count) only (a sub-mix; count = 1: one filtered stream).  *out_frames, and the capacity dst
 * needs, stay those of the whole batch: the frames behind the subset's last source are silence (zeros). */
rh_status rh_rlm_run_subset(rh_rlm *p, uint32_t first, uint32_t count, float *dst,
                            uint64_t out_capacity_frames, uint64_t *out_frames, rh_stream stream);
/* Block streaming of the fused path: the same sources arrive block by block (what a `GpuMixer` shim does
 * with its upstream iterators).  begin() starts a stream; every block() call passes, per source, a device
 * pointer to `avail_frames` input frames that start where the previous call's *consumed_frames left off
 * (the caller keeps the unconsumed frames in front of the new ones), and receives *out_frames mixed frames
 * in dst.  flush != 0 ends the stream (rodio's None): the remaining frames and the verbatim last frame are
 * emitted.  Across blocks the handle carries the converter's position and the summed filter state; the
 * concatenated output equals one rh_rlm_run over the whole stream to f32 rounding (<= 1e-6 in the tests).
 * *consumed_frames is always a whole number of 16-byte vectors (a multiple of 2 stereo / 4 mono frames): a caller whose sources are
 * RESIDENT in device memory passes `row + consumed so far` as the next block's pointer -- no staging copy at all (bench.py --config stream).
 * cfg.span_len != 0: every source reports spans of that many samples (a SamplesBuffer longer than 32 768 samples: any
 * span_len >= 32768): the converter restarts every min(span_len, 32768) samples at the same frames of every source
 * (uniform.rs:56-67), each span's last frame verbatim.  Sources with other span patterns: rh_uniform_segments in front of a
 * pass-through stream (from_rate == to_rate), which is what include/rodio_hip.hpp does.  One set of sources per stream.
 * Both block entries stage their descriptors in a ring of four page-locked slots per handle: of blocks queued back to back on a
 * stream that is backed up, the fifth waits until the copy of the first has run. */
rh_status rh_rlm_stream_begin(rh_rlm *p);
rh_status rh_rlm_stream_block(rh_rlm *p, const float *const *srcs_host, uint32_t n_sources,
                              uint64_t avail_frames, int32_t flush, float *dst,
                              uint64_t out_capacity_frames, uint64_t *out_frames,
                              uint64_t *consumed_frames, rh_stream stream);
/* The same for sources that end at different times (what a mixer usually holds): source s passes
 * avail_frames_host[s] frames; ended_host[s] != 0 says that these are its last ones (rodio's None; sticky).
 * All sources run on one clock (they start with the stream).  Live sources bound what a block can emit (whole
 * tiles of 64*frames_per_lane output frames; everything once all sources have ended, which ends the stream);
 * *consumed_frames is common to all sources: each drops min(consumed, what it holds).  The handle keeps one
 * filter state PER SOURCE across blocks (this entry always takes the ragged-batch kernel).  begin() as above;
 * a stream uses one of the two block entries throughout. */
rh_status rh_rlm_stream_block_v(rh_rlm *p, const float *const *srcs_host, const uint64_t *avail_frames_host,
                                const uint8_t *ended_host, uint32_t n_sources, float *dst,
                                uint64_t out_capacity_frames, uint64_t *out_frames,
                                uint64_t *consumed_frames, rh_stream stream);
/* rh_rlm_stream_block_v, sources that RUN TOGETHER: while every source is live and passes the same number of frames -- what a mixer's
 * sources do from the moment they are added until the first of them ends -- their filter states need not be told apart: the stream
 * carries their SUM (as rh_rlm_stream_block does) and every block is summed at the input rate first and converted and filtered once
 * (DESIGN.md 4.6).  When a source ends or falls behind, the states of the others are recovered from the rows of the block BEFORE
 * (a replay of its last few tiles through the per-source kernel: a stable filter has forgotten what lies further back) and the stream
 * goes on with one state per source -- until its sources run together AGAIN: every source either gone (ended, and everything it had
 * emitted) or live with the same frames as the other live ones.  Then the sum of the live states becomes the stream's summed state and
 * the blocks are summed first once more (a block with a state per source costs a wave per tile walking every source: ~360 us for 256
 * sources whatever the block's length; a mixer whose sounds end one after the other would otherwise spend its life there).
 * The caller opts in by promising what the recovery needs: on != 0 = "the rows I pass to a block
 * stay valid and unchanged until the work of the NEXT block call has run" (three row sets in rotation do: include/rodio_hip.hpp).
 * Between rh_rlm_stream_begin and the stream's first block.  Without it -- the default -- every block takes the per-source kernel. */
rh_status rh_rlm_stream_keep_history(rh_rlm *p, int32_t on);
/* Blocks side by side.  A block of a stream on the summed state is ONE launch where the library can make it one (k_rlm_sblk: the sum over
 * the sources, the conversion and the filter in one kernel), and a short kernel spends a third of its life filling and draining the chip.
 * on != 0 = "the rows I pass to a block call are COMPLETE in device memory when I make the call, and nothing I queued on `stream` since the
 * block in front is something this block has to wait for" (decoded assets resident in HBM; a caller that has synchronised its producer).
 * The library then launches a block WITHOUT a barrier behind the block in front, on the same stream (hipExtAnyOrderLaunch): its workgroups
 * start on every XCD that has finished the block in front while the others still work on it, and the few tiles the stream's filter state
 * still reaches wait for it inside the kernel (tagged words, left by the last tile of the block in front).  Nothing changes for the output:
 * a block's dst is complete in the order of the stream for every later launch that carries a barrier -- every launch but these.  Off (the
 * default: rows that a copy on the caller's stream is still filling) every block starts behind everything in front of it.
 * rh_rlm_set_exclusive(0) switches it off (the blocks' workgroups must fit the chip at once). */
rh_status rh_rlm_stream_overlap(rh_rlm *p, int32_t on);
/* Diagnostics: blocks of the current stream that ran as one launch. */
rh_status rh_rlm_stream_one_launch_blocks(rh_rlm *p, uint32_t *blocks);
/* Diagnostics: ... and how many of those started while the block in front still ran (rh_rlm_stream_overlap). */
rh_status rh_rlm_stream_overlapped_blocks(rh_rlm *p, uint32_t *blocks);
/* Diagnostics: blocks of the current stream that ran on the summed state / on one state per source, and recoveries in between. */
rh_status rh_rlm_stream_stats(rh_rlm *p, uint32_t *summed_blocks, uint32_t *per_source_blocks, uint32_t *recoveries);
/* No mixer: every source is converted and filtered into its own row, dst + s*dst_stride_frames*channels
 * (equal-length STEREO sources only: RH_ERR_UNSUPPORTED otherwise; with more than one source dst_stride_frames is even and at least
 * *out_frames: RH_ERR_INVALID otherwise -- every row starts on a 16-byte boundary).  One launch for all sources. */
rh_status rh_rlm_run_batch(rh_rlm *p, float *dst, uint64_t dst_stride_frames, uint64_t *out_frames,
                           rh_stream stream);
/* Optional: time the candidate launch geometries of the equal-length kernel on the sources that are set
 * (a few runs each into dst, which is overwritten) and keep the fastest -- like a GEMM library's
 * find step.  Synchronises.  Works on whichever kernel the current sources take.  Reports the geometry kept. */
rh_status rh_rlm_autotune(rh_rlm *p, float *dst, uint64_t out_capacity_frames, rh_stream stream,
                          uint32_t *frames_per_lane, uint32_t *ring_stages);
/* After a synchronise: 0 if the last run completed, RH_ERR_TIMEOUT if a bounded wait expired. */
rh_status rh_rlm_last_status(rh_rlm *p);
/* Diagnostics: number of (tile, source) carries since the last call that had not been published by
 * the neighbouring tile when they were due and had to be polled (synchronises with the device). */
rh_status rh_rlm_late_carries(rh_rlm *p, uint64_t *count);
/* Diagnostics, only in builds with -DRH_PHASE_PROFILE (RH_ERR_UNSUPPORTED otherwise): mean shader
 * cycles per wave spent in each phase of the source loop during the last run. */
rh_status rh_rlm_phase_cycles(rh_rlm *p, double out8[8]);
/* Launch geometry chosen by create (for the bench's roofline report). */
typedef struct rh_rlm_geometry_info {
    uint32_t threads;          /* lanes per workgroup (one wave64 = one time tile) */
    uint32_t frames_per_lane;  /* tile = 64 * frames_per_lane output frames */
    uint32_t ring_stages;      /* sources prefetched ahead + 1 */
    uint32_t stage_kib;        /* KiB of LDS per stage */
    uint32_t lds_bytes;        /* dynamic LDS per workgroup */
    uint32_t lookback_tiles;   /* predecessor tiles whose aggregates form a tile's carry */
    uint32_t resident_waves_per_cu;
    uint32_t n_tiles;          /* grid of the last set_sources */
    uint32_t general_kernel;   /* 1: ragged-batch kernel (per-source carries), 0: equal-length kernel */
    uint32_t ragged_pair;      /* 1: one-shot runs of this batch take k_rlm_fast<RAG> (stable sources summed first, the pairs of ending sources behind them) instead of the ragged-batch kernel */
    uint32_t mix_first;        /* one-shot runs of this batch (filtered, equal lengths) sum the sources at the input rate first and convert + filter
                                * that one stream: 1 = two launches (k_mix_ring or k_mix_rows, then the fused kernel on one source),
                                * 2 = one (k_rlm_chunk: long stereo rows); 3 = a handle with a filter per source (rh_rlm_set_filters) whose classes all take
                                * k_rlm_chunk and whose LAST run walked them in one launch (k_rlm_chunk_multi), the classes' mixes added behind it */
} rh_rlm_geometry_info;
rh_status rh_rlm_geometry(rh_rlm *p, rh_rlm_geometry_info *info);

/* ---- sources that start on the device: rodio's synthetic generators.  Nothing is pulled from the host or uploaded.
 * SignalGenerator::new(rate, freq, Function) (src/source/signal_generator.rs:86-154) and SineWave / SquareWave /
 * TriangleWave / SawtoothWave::new(freq) (sine.rs, square.rs, triangle.rs, sawtooth.rs: the same at DEFAULT_SAMPLE_RATE,
 * 48 kHz).  A generator is its state, two floats: phase_step = 1 / (rate as f32 / freq) and the phase of the NEXT sample;
 * and its function (RH_GEN_*).  init (host): the state of a new generator (phase 0); refuses freq <= 0 and NaN (the reference's assert!); +inf gives a NaN phase, as the reference's.  seek: try_seek,
 * (as_secs_f32(pos) * rate as f32 / period).rem_euclid(1.0) (signal_generator.rs:148-153).  advance (host): the phase n
 * samples on, bit for bit n steps of `(phase + phase_step).rem_euclid(1.0)` (signal_generator.rs:137), in far fewer steps.
 * generate: row g of dst (dst + g * ld, ld >= n) receives the next n samples of generator g < n_gens (<= 65535), whose
 * state is states_dev[2g .. 2g+1] and function functions_dev[g] (both DEVICE arrays); its phase moves on by n: the next
 * call continues the stream.  Triangle, square and sawtooth are the reference's
 * bits; sine is sinf of the reference's f32 argument.  A function code outside RH_GEN_* gives NaN samples.  dst
 * must not alias the states or functions. */
enum { RH_GEN_SINE = 0, RH_GEN_TRIANGLE = 1, RH_GEN_SQUARE = 2, RH_GEN_SAWTOOTH = 3 };
rh_status rh_signal_generator_init(float state_host[2], uint32_t sample_rate, float frequency);
rh_status rh_signal_generator_seek(float *phase_host, uint32_t sample_rate, float frequency, uint64_t pos_ns);
float rh_signal_phase_advance(float phase, float phase_step, uint64_t n);
rh_status rh_signal_generate(float *dst, uint64_t ld, uint64_t n, float *states_dev, const int32_t *functions_dev,
                             uint32_t n_gens, rh_stream stream);
/* chirp(rate, f0, f1, duration) (src/source/chirp.rs:11-97).  total_samples: (duration.as_secs_f64() * rate as f64) as u64
 * (chirp.rs:36-44).  total_duration: Duration::from_secs_f64(total / rate) (chirp.rs:83-86), rounded to the nanosecond.
 * rh_chirp: samples first .. first + n of the sweep (sample i: sin((i / rate) as f32 * TAU * freq_i), freq_i between f0 and f1
 * by (i / total) as f32, chirp.rs:53-63); *out_n = what is left of it, at most n (the iterator ends at total).  Any
 * u64 position: a seek is `first` (chirp.rs:88-96: min(pos * rate, total)). */
rh_status rh_chirp_total_samples(uint32_t sample_rate, uint64_t duration_ns, uint64_t *total);
rh_status rh_chirp_total_duration(uint32_t sample_rate, uint64_t total, uint64_t *secs, uint32_t *nanos);
rh_status rh_chirp(float *dst, uint64_t first, uint64_t n, uint64_t total, uint32_t sample_rate, float start_frequency,
                   float end_frequency, uint64_t *out_n, rh_stream stream);

/* ---- noise sources that start on the device: rodio's noise.rs (feature `noise`): WhiteUniform, WhiteTriangular, WhiteGaussian, Pink, Blue,
 * Violet, Brownian, Red, Velvet -- mono, endless.  The noise is rh_dither's counter-based generator (above): h(seed, k) = mix(seed ^ mix(k + 1)),
 * W(k) = u1(h(seed, k)); sample k (a u64, 0 at init, past 2^32 as needed) of a stream is
 *   WHITE_UNIFORM W(k); WHITE_TRIANGULAR (u1 + u2) * 0.5; WHITE_GAUSSIAN rh_dither's GPDF (sigma 0.6) -- each of h(seed, k);
 *   BLUE W(k) - W(k-1), W(-1) = 0; VIOLET B(k) - B(k-1), B = BLUE, B(-1) = 0;
 *   PINK ((..((0 + v0) + v1) ..) + v15) / 16, v_i = 0 if k < 2^i, else W(D(m) + i), m = k & ~(2^i - 1), D(m) = sum_{j<16} floor((m-1) / 2^j)
 *        (W indexed by draw number: noise.rs:491-512's counters in closed form);
 *   VELVET(density) grid = ceil(rate as f32 / density as f32); cell c = k / grid, hc = h(seed, c): the impulse sits at
 *        (u32(hc >> 32) * grid) >> 32, +1 if bit 31 of hc is set, else -1; every other sample +0.0;
 *   RED acc = acc * leak + W(k); out = acc * scale, leak = 1 - (2 PI 5) / rate, scale = 1 / sqrt((s s) / (1 - leak leak)), s = sqrt(1/3);
 *   BROWNIAN the same over WHITE_GAUSSIAN, s = 0.6.  (noise.rs:680-712; all f32.)
 * The white kinds, blue, violet, pink and velvet are exact; the integrators run as a time-parallel scan, within 4e-5 absolute of the f64
 * recurrence on the same white samples.
 * init (host): the eight state words of a new stream -- [0..1] seed (lo, hi), [2..3] the next k (lo, hi) = 0, [4] kind, [5] velvet: grid
 * (lo) / red, brownian: leak (f32 bits), [6] velvet: grid (hi) / red, brownian: scale (f32 bits), [7] acc (f32 bits) = 0.  An unknown
 * kind, rate 0 or a velvet density of 0 (rodio's NonZero) is RH_ERR_INVALID.  try_seek is a host edit of the words: rodio's changes nothing
 * but an integrator's acc, which it sets to 0 (noise.rs:795-799, 875-879); k is not moved.
 * generate: row g of dst (dst + g * ld, ld >= n, any alignment) receives the next n samples of stream g < n_streams (<= 65535), whose eight
 * words are states_dev[8g .. 8g+7] (a DEVICE array); any mix of kinds in one call.  k moves on by n and acc is carried on the device: the next
 * call continues every stream.  A kind outside RH_NOISE_* gives NaN samples.  dst must not alias the states. */
enum {
    RH_NOISE_WHITE_UNIFORM = 0,
    RH_NOISE_WHITE_TRIANGULAR = 1,
    RH_NOISE_WHITE_GAUSSIAN = 2,
    RH_NOISE_PINK = 3,
    RH_NOISE_BLUE = 4,
    RH_NOISE_VIOLET = 5,
    RH_NOISE_BROWNIAN = 6,
    RH_NOISE_RED = 7,
    RH_NOISE_VELVET = 8
};
rh_status rh_noise_init(uint32_t state_host[8], int32_t kind, uint32_t sample_rate, uint64_t seed, uint32_t density);
rh_status rh_noise_generate(float *dst, uint64_t ld, uint64_t n, uint32_t *states_dev, uint32_t n_streams, rh_stream stream);

/* ---- multi-GPU: one process per GPU, sources sharded over the ranks, the mixer sum (src/mixer.rs:185-198 is the
 * only place rodio's streams meet) completed by ONE collective per mixed block over RCCL / xGMI.  Rank 0 calls
 * rh_comm_unique_id and hands the 128 bytes to the other ranks (any out-of-band channel); every rank then calls
 * rh_comm_init on its own device.  all-reduce leaves the full mix on every rank; reduce only on `root` (the
 * rank that owns the sink).  Both run in place on `stream`, behind the kernel that produced the block. */
typedef struct rh_comm rh_comm;
rh_status rh_comm_unique_id(uint8_t out128[128]);
rh_status rh_comm_init(rh_comm **out, int32_t rank, int32_t nranks, const uint8_t uid128[128]);
rh_status rh_comm_destroy(rh_comm *c);
rh_status rh_allreduce_sum_f32(rh_comm *c, float *buf, size_t n, rh_stream stream);
rh_status rh_reduce_sum_f32(rh_comm *c, float *buf, size_t n, int32_t root, rh_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* RODIO_HIP_H */
