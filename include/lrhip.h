/*
 * lrhip.h - C ABI of liblrhip.so, the MI355X (gfx950) DSP block engine behind LuaRadio's block API.
 *
 * This is the drop-in boundary: what a LuaJIT `ffi.cdef` (see INTEGRATION.md and lua/radio/) binds in
 * place of the VOLK / liquid-dsp / FFTW3f entry points the reference's blocks call from process().
 * Plain pointers and sizes only; no C++ or torch types.  All paths below are relative to /root/reference.
 *
 * Conventions (liquid-dsp style, as used by the reference at radio/blocks/signal/firfilter.lua:167-226):
 *   - `T *q = lrhip_X_create(params)` returns NULL on error (the reference's blocks then raise
 *     `error("Creating ... object")`, firfilter.lua:199-201); `lrhip_strerror()` gives the text.
 *   - `lrhip_stage_execute(q, in, n, out, cap)` is one block's process(): host pointers in, host pointers
 *     out, returns the number of output samples written (>= 0) or < 0 on error.  All cross-call state
 *     (FIR history, rotator phase, downsampler index, discriminator previous sample, IIR state) lives in
 *     the stage object on the device, so arbitrary chunking gives identical sample values for every block on
 *     its own in direct form (the property tests/jigs.lua:213-250 pins with one-sample chunks).  Overlap-save
 *     filters and the fused forms a DEFAULT chain takes (listed at lrhip_chain_create) agree across chunkings
 *     to Float32 rounding (<= 1e-6 / 2e-7), not bit for bit; lrhip_chain_create_ex(.., LRHIP_CHAIN_EXACT)
 *     restores the bits.
 *   - `lrhip_stage_destroy(q)` is bound with ffi.gc.
 *   - Sample layouts are the reference's: ComplexFloat32 = struct{float real, imag} (8 B, interleaved,
 *     radio/types/complexfloat32.lua:19-24), Float32 = struct{float value} (4 B, radio/types/float32.lua:17-21).
 *   - Nothing here throws, aborts or prints.  Single-threaded use per process, like a LuaRadio block
 *     (one process per block after fork(): radio/core/composite.lua:569); lrhip_init() must first be
 *     called AFTER fork (it creates the HIP context lazily on first use).
 */
#ifndef LRHIP_H
#define LRHIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrhip_stage lrhip_stage_t;   /* one block's device state + kernels */
typedef struct lrhip_chain lrhip_chain_t;   /* a linear run of stages with device-resident edges */

/* ---- runtime -------------------------------------------------------------------------------------- */
/* Select the device and create the stream.  Replaces platform.load()/feature detection for a native
 * library (radio/core/platform.lua:277-299).  device < 0 => current device.  Idempotent. */
int lrhip_init(int device);
/* Text of the last error on this thread ("" if none). */
const char *lrhip_strerror(void);
/* Number of visible HIP devices (for the fan-out scheduler), or < 0 on error. */
int lrhip_device_count(void);
/* The device this process's library is bound to (what lrhip_init chose; the dst_device / src_device of lrhip_peer_copy), -1 before the
 * first lrhip_init / stage creation.  One device per process: after a successful lrhip_init(d) a later lrhip_init(d2) with d2 >= 0 and
 * d2 != d fails - LuaRadio runs one process per block (radio/core/composite.lua:569), so "a branch per GPU" is "a device per process". */
int lrhip_device(void);
/* Launch all subsequent work on an externally owned hipStream_t (NULL => the library's own non-blocking stream; HIP's explicit handles
 * hipStreamLegacy = (hipStream_t)1 and hipStreamPerThread = (hipStream_t)2 are accepted - a host that keeps its vectors on the default
 * stream passes 1).  Work already queued on the previous stream is ordered before whatever follows on the new one. */
int lrhip_set_stream(void *hip_stream);
/* Block until everything queued by this library has finished. */
int lrhip_synchronize(void);
/* Library version string. */
const char *lrhip_version(void);

/* ---- stage constructors ---------------------------------------------------------------------------- */
/* FIRFilterBlock (firfilter.lua:43-74 instantiate, :90-163 / :230-305 dot-product form, :320-398 overlap-save
 * framing).  taps: ntaps floats (taps_complex = 0) or ntaps {re,im} pairs (taps_complex = 1), in the
 * reference's natural order h[0..M-1] (the library reverses them, :234-238).  input_complex selects
 * ComplexFloat32 or Float32 samples; complex taps require complex input (:69-74).
 * decim >= 1 fuses a following DownsamplerBlock(decim) (radio/composites/decimator.lua:37-39): only every
 * decim-th filter output is computed and emitted, with the downsampler's carried phase index.
 * use_fft: 0 = direct form (bit-identical to the fmaf chain in the reference's tap order);
 *          1 = overlap-save as the reference runs it (:320-398): only whole L = N-M+1 blocks are emitted,
 *              N = 2^floor(log2(8M)), the tail is retained; arithmetic by the fused FFT kernel for 32 <= M <= 8192;
 *          2 = overlap-save arithmetic, 32 <= M <= 8192, with sample-exact emission (every call returns one output per input, like
 *              the direct form) - the fast path: the fused 1024-point kernel to 512 taps, 4096-point blocks above (one per wave as
 *              64 x 64 - real or complex taps on a ComplexFloat32 stream, real taps on a Float32 stream; two partitions per launch
 *              above 2 049 taps, two launches above 4 097), <= 1e-6 of the exact result whichever kernel the launch size selects;
 *          3 = automatic: 2 when the filter qualifies and has at least 48 taps (where the FFT form is the faster one on
 *              MI355X), else 0.  Outside the stated tap range 1 and 2 keep their emission rule and use the direct arithmetic. */
lrhip_stage_t *lrhip_fir_create(const float *taps, unsigned ntaps, int taps_complex, int input_complex,
                                unsigned decim, int use_fft);
/* FrequencyTranslatorBlock (radio/blocks/signal/frequencytranslator.lua:26-53, :93-110):
 * y[n] = x[n] * exp(j*omega*n), omega = 2*pi*offset/rate computed by the caller as at :95. */
lrhip_stage_t *lrhip_rotator_create(double omega);
/* DownsamplerBlock (radio/blocks/signal/downsampler.lua:29-56). elem_size = 8 (ComplexFloat32) or 4 (Float32). */
lrhip_stage_t *lrhip_downsampler_create(unsigned factor, int elem_size);
/* FrequencyDiscriminatorBlock (radio/blocks/signal/frequencydiscriminator.lua:25-38, :48-88).
 * gain = 2*pi*modulation_index (:28).  ComplexFloat32 in, Float32 out. */
lrhip_stage_t *lrhip_fmdiscrim_create(double gain);
/* IIRFilterBlock (radio/blocks/signal/iirfilter.lua:39-61, :113-181): b[nb] feed-forward, a[na] feedback
 * (a[0] divides).  SinglepoleLowpassFilterBlock / FMDeemphasisFilterBlock compute b,a on the host
 * (singlepolelowpassfilter.lua:55-67) and call this with nb = na = 2. */
lrhip_stage_t *lrhip_iir_create(const float *b, unsigned nb, const float *a, unsigned na, int input_complex);
/* spectrum_utils.PSD (radio/utilities/spectrum_utils.lua:522-561, :585-640) over frames of n samples:
 * window multiply -> n-point DFT -> |X|^2/scale -> optional 10*log10 -> optional fftshift (:654-667).
 * window: n floats (the caller builds the periodic window as at :547); scale = sample_rate * sum(w^2) (:597).
 * Input n_in must be a multiple of n; output is n_in Float32 values.  n must be a power of two, 8..4096. */
lrhip_stage_t *lrhip_psd_create(unsigned n, const float *window, double scale, int logarithmic,
                                int input_complex, int fftshift);
/* spectrum_utils.DFT / IDFT (spectrum_utils.lua:25-113, :259-349) over frames of n samples.
 * inverse != 0 applies the 1/n normalisation (:335-338).  real_side: for forward transforms a Float32 input,
 * for inverse transforms a Float32 output (real part, :499-503).  Complex side is ComplexFloat32. */
lrhip_stage_t *lrhip_dft_create(unsigned n, int inverse, int real_side);

/* IQFileSource / RealFileSource sample conversion (radio/blocks/sources/iqfile.lua:99-113, realfile.lua:99-110,
 * formats table radio/utilities/format_utils.lua:82-97): raw file samples -> (value - offset)/scale.
 * format: "u8","s8","u16le","u16be","s16le","s16be","u32le","u32be","s32le","s32be","f32le","f32be","f64le","f64be".
 * complex_out != 0: input is interleaved I/Q (2 raw scalars per sample), output ComplexFloat32; else Float32.
 * Input samples are the RAW file records (lrhip_stage_input_size() bytes each), so the bytes read from the file
 * are handed over unchanged and converted on the device. */
lrhip_stage_t *lrhip_format_convert_create(const char *format, int complex_out);
/* The sink direction (radio/blocks/sinks/iqfile.lua:68-85, realfile.lua): ComplexFloat32 / Float32 samples -> raw file records
 * raw = x*scale + offset stored into the format's type (C conversion, i.e. truncation for the integer formats), byte-swapped
 * for the big-endian formats.  Output samples are lrhip_stage_output_size() bytes each. */
lrhip_stage_t *lrhip_format_pack_create(const char *format, int complex_in);

/* Two-input element-wise blocks: op = "multiply" (radio/blocks/signal/multiply.lua:43-76), "multiplyconjugate"
 * (multiplyconjugate.lua:41-59, complex only), "add" (add.lua), "subtract" (subtract.lua), "floattocomplex" (floattocomplex.lua: two Float32 inputs ->
 * ComplexFloat32 (in1, in2); input_complex ignored).  Replaces
 * volk_32fc_x2_multiply_32fc_a / volk_32f_x2_multiply_32f_a / volk_32fc_x2_multiply_conjugate_32fc_a.
 * op = "sampler" (radio/blocks/signal/sampler.lua:33-53): in1 = data (ComplexFloat32 if input_complex, else Float32), in2 = a Float32
 * clock (4 B whatever the data type); emits data[i] where clock[i] > 0 and the last clock sample != 0 before it was < 0 (initial state LOW).
 * The output count depends on the clock: at most ceil(n/2) + 1 = lrhip_stage_max_output(); the call returns the exact count.
 * Executed with lrhip_stage_execute2*(). */
lrhip_stage_t *lrhip_binary_create(const char *op, int input_complex);

/* MultiplyConstantBlock (radio/blocks/signal/multiplyconstant.lua:28-71): real constant (constant_complex = 0, `im`
 * ignored) on Float32 or ComplexFloat32 input, or a complex constant on ComplexFloat32 input only (:42-44). */
lrhip_stage_t *lrhip_multiply_constant_create(float re, float im, int constant_complex, int input_complex);
/* UpsamplerBlock (radio/blocks/signal/upsampler.lua:26-53): zero-stuffing by `factor`. elem_size = 8 or 4. */
lrhip_stage_t *lrhip_upsampler_create(unsigned factor, int elem_size);

/* FrequencyModulatorBlock (radio/blocks/signal/frequencymodulator.lua:24-90; replaces freqmod_create / freqmod_modulate_block
 * :33-51): Float32 in, ComplexFloat32 out = exp(j * running phase), phase += 2*pi*modulation_index*x[n]. */
lrhip_stage_t *lrhip_fmmod_create(double modulation_index);

/* AGCBlock (radio/blocks/signal/agc.lua:25-96).  power_alpha = 1/(1 + power_tau*rate), gain_alpha = 1/(1 + gain_tau*rate)
 * (:46-49), target / threshold LINEAR power (10^(dB/10), :53-55).  Both recurrences run as parallel scans in double. */
lrhip_stage_t *lrhip_agc_create(double power_alpha, double gain_alpha, double target, double threshold, int input_complex);

/* PowerSquelchBlock (radio/blocks/signal/powersquelch.lua:26-80): alpha = 1/(1 + tau*rate), threshold LINEAR power; samples
 * pass while the running average power is at or above the threshold, else zeros. */
lrhip_stage_t *lrhip_powersquelch_create(double alpha, double threshold, int input_complex);

/* One-input element-wise blocks. op: "complexmagnitude", "complexphase", "complextoreal", "complextoimag",
 * "complexconjugate" (ComplexFloat32 in), "realtocomplex", "absolutevalue" (Float32 in), and "addconstant"
 * (radio/blocks/signal/addconstant.lua:26-75: constant (re, im); constant_complex / input_complex as for
 * lrhip_multiply_constant_create).  For the ops with a fixed input type input_complex is ignored.
 * Every other block created here carries its parameters in the op string, "name:key=value:key=value": the fields in any order, each key once
 * (luaradio_amd/csrc/op_string.h reads them all; doubles as %.17g / repr(float) text through strtod, integers in decimal, lists of Float32 values
 * separated by commas; re / im / constant_complex / input_complex ignored; a malformed field, an unknown, repeated or missing key or a value of
 * the wrong kind returns NULL with an lrhip_strerror() message, before the device is touched).  All exact (compared with ==), state carried across calls:
 *   "zerocrossingclockrecovery:period=P:threshold=T"  (zerocrossingclockrecovery.lua:35-73, P = rate / baudrate) Float32 -> +-1 Float32
 *   "slicer:threshold=T"                               (slicer.lua) Float32 -> Bit (1 B): x > T in double
 *   "differentialdecoder:invert=0|1"                   (differentialdecoder.lua) Bit -> Bit: prev ^ x, or (prev ^ x + 1) % 2; prev = last input byte
 *   "clocksampler:period=P:threshold=T"                sampler(data = x, clock = zerocrossingclockrecovery(x)) as one stage, Float32 -> Float32,
 *                                                      count data-dependent (<= ceil(n/2) + 1).  In a chain a slicer [and a differentialdecoder]
 *                                                      right after it run in its final pass (Bit out), except with LRHIP_CHAIN_NO_FUSION;
 *                                                      the fused stage continues the carried state of the caller's clocksampler and decoder.
 *   "binaryphasecorrector:num_samples=N[:sample_interval=I]"  (binaryphasecorrector.lua:43-73, I defaults to 32) ComplexFloat32 -> ComplexFloat32:
 *                                                      x * (cos(-avg), sin(-avg)) rounded to ComplexFloat32, avg = the mean of the phases (clamped to
 *                                                      [-pi/2, pi/2]) measured at the absolute samples 0, I, 2I, ... over the last N measurements (a window
 *                                                      that starts as N zeros), in exact fixed-point sums: bit-identical however the stream is cut.  N in
 *                                                      [1, 2^24], I in [1, 2^31], integers.  A NaN phase makes every later output NaN until reset.
 *                                                      memory() = N I.  In a chain a complextoreal right after it runs in its rotation pass (Float32 out).
 *   "preamblesampler:period=T:num_samples=N:preamble=0101..."  (preamblesampler.lua:49-138; T = floor(rate / baudrate), the preamble a string of
 *                                                      0 / 1 characters, T and N integers) Float32 -> Float32: finds the preamble at one tap per symbol,
 *                                                      moves on while its energy (a double sum in tap order) does not degrade, then emits N samples T
 *                                                      apart; count data-dependent (<= ceil(n/2) + 1, <= n for T = 2).  Refused: T < 2 and N < 2 (the
 *                                                      reference never leaves its sampling state), an empty preamble, a character other than 0 / 1, and a
 *                                                      buffer 2^ceil_log2(T L + 1) above 2^21 samples (every T L <= 2^20 is admitted).  The carried
 *                                                      state is the last 2^ceil_log2(T L + 1) samples and the automaton's state.
 *   "manchesterdecoder:invert=0|1"                     (manchesterdecoder.lua:31-61) Bit -> Bit (input bytes read as & 1): a 0,1 pair gives 0 ^ invert, a
 *                                                      1,0 pair 1 ^ invert, an equal pair is a clock slip and the newer bit stays pending; count
 *                                                      data-dependent (<= (n + 1) / 2).
 *   "varicodedecoder"                                  (varicodedecoder.lua:61-87; no parameters, any is refused) Bit -> Byte (one uint8_t per
 *                                                      character): every byte joins a state; when the state's last two bytes both equal 0 the L - 2
 *                                                      bytes in front of them (L = the state's length, 2 .. 11) are read as a number, most significant
 *                                                      first, and its character in the PSK31 Varicode alphabet, if it has one, is emitted; the state is
 *                                                      emptied there, and also once it holds more than 10 bytes.  Bytes are read as the reference reads
 *                                                      them: a byte is a delimiter zero only when it equals 0 and a one only when it equals 1, so 2 or
 *                                                      255 breaks a delimiter and counts as a 0 in the number.  As in the reference the 40 codes of 10
 *                                                      bits (`Z`, `?`, ...) are never decoded: the state is emptied at length 11, in front of their
 *                                                      second delimiter zero, and the first one stays behind in the new state, which costs the next
 *                                                      character a bit of room - a 9-bit code right behind a lost character is lost too ("!Zx" gives
 *                                                      "!x").  Count data-dependent (<= min(n, (n + 10) / 3): a character owns a code bit and 00, its
 *                                                      second zero lies in the call, at most 10 bytes are carried in); the carried state is the state's
 *                                                      length (0 .. 10) and its raw bytes; reset empties it; bit-identical however the stream is cut.
 *                                                      Fuses with nothing.
 *   "rdsframer"                                        (rdsframer.lua:95-201; no parameters, any is refused) Bit -> 8-byte records
 *                                                      {uint16_t blocks[4]}, little-endian: the data words A, B, C, D of every 104-bit window whose four
 *                                                      26-bit blocks have a zero or single-bit-error syndrome under the offset words A, B, C (C' only
 *                                                      when C is uncorrectable) and D, single-bit errors corrected.  A byte counts as 1 only when it
 *                                                      equals 1.  Windows are tested from the first bit no accepted frame has consumed; an accepted
 *                                                      frame moves that bit 104 on, so a valid window inside an accepted frame is not emitted.  Count
 *                                                      data-dependent (<= (n + 103) / 104); the carried state is the at most 103 bits since that bit;
 *                                                      bit-identical however the stream is cut.  Fuses with nothing.
 *   "scmframer" | "scmplusframer" | "idmframer"        (scmframer.lua:166-211, scmplusframer.lua:181-225, idmframer.lua:187-243; no parameters, any is
 *                                                      refused) Bit -> one little-endian record per frame, pad bytes zero, numeric fields the
 *                                                      reference's Bit.tonumber values:
 *                                                        struct lrhip_scm_frame {       16 bytes, per 96-bit window
 *                                                          uint32_t ert_id, consumption; uint16_t crc;
 *                                                          uint8_t ert_type, physical_tamper, encoder_tamper, reserved, pad[2]; };
 *                                                        struct lrhip_scmplus_frame {   16 bytes, per 128-bit window
 *                                                          uint32_t ert_id, consumption; uint16_t tamper, crc;
 *                                                          uint8_t protocol_id, ert_type, pad[2]; };
 *                                                        struct lrhip_idm_frame {       88 bytes, per 736-bit window
 *                                                          uint32_t ert_id, last_consumption_count;
 *                                                          uint16_t transmit_time_offset, serial_crc, packet_crc;
 *                                                          uint8_t application_version, ert_type, consumption_interval_count, module_programming_state;
 *                                                          uint8_t tamper_count[6], async_count[2], power_outage_flags[6],
 *                                                                  differential_consumption_intervals[53], pad[3]; };
 *                                                      (the byte arrays as Bit.tobytes packs them: MSB first, in frame order).  A window is a frame
 *                                                      when it starts with the preamble / sync word (21 bits 0x1f2a60, 16 bits 0x16a3, 32 bits
 *                                                      0x555516a3), the codeword behind it (75, 112, 704 bits) has a zero or single-bit-error syndrome
 *                                                      (the erroneous byte b replaced by (~b) & 1), and then protocol_id == 0x1e (SCM+) or packet type
 *                                                      0x1c, length 0x5cc6 and serial CRC (IDM) hold.  A byte counts as 1 only when it equals 1; the
 *                                                      IDM serial CRC alone reads byte values as idm_compute_crc does.  As in the reference the
 *                                                      correction is made in the buffer: an SCM+ / IDM window that corrects a byte and then fails its
 *                                                      later check is rejected with the corrected byte left for the windows after it.  An accepted
 *                                                      frame moves the search L bits on.  Count data-dependent (<= (n + L - 1) / L); the carried
 *                                                      state is the at most L - 1 bytes (corrections applied) since the first bit no accepted frame
 *                                                      has consumed; bit-identical however the stream is cut.  Fuses with nothing.
 *   "ax25framer"                                       (ax25framer.lua:94-284; no parameters, any is refused) Bit -> one little-endian record per frame,
 *                                                      pad bytes and the tail of `data` behind `length` zero:
 *                                                        struct lrhip_ax25_frame {      416 bytes
 *                                                          uint16_t length;             octets in data: the unstuffed frame without its FCS, 13 .. 396
 *                                                          uint16_t crc;                the received FCS, Bit.tonumber(frame, len - 16, 16, "lsb")
 *                                                          uint8_t num_addresses;       addresses ax25_extract_frame walked (7 octets each, from data[0])
 *                                                          uint8_t control, pid;        pid 0 when absent
 *                                                          uint8_t has_pid;             0 when the reference's pid and payload are nil, else 1 (the
 *                                                                                       payload may then be "")
 *                                                          uint16_t payload_offset, payload_length;     the payload inside data
 *                                                          uint8_t pad[4], data[400]; };                each octet Bit.tonumber(.., 8, "lsb")
 *                                                      The consumed flags are the chain "first 8 bytes that read 0x7e at or after q, then q = p + 8";
 *                                                      the bytes between two consecutive consumed flags are a frame when the segment before them was
 *                                                      not emitted (the reference is IDLE behind a frame: one that shares its opening flag with an
 *                                                      emitted frame's closing flag is lost), they are at most 3185, and unstuffed they are whole
 *                                                      octets, at least 120 bits, the FCS matches and the address chain, the control octet and the
 *                                                      optional PID / payload extract.  Bytes are read as the reference reads them: a byte is a 1 for
 *                                                      the flag and the octets only when it equals 1; a byte is unstuffed only when it equals 0 behind
 *                                                      exactly five bytes equal to 1; the CRC feeds back only when (crc & 1) ^ value == 1.  Count
 *                                                      data-dependent (<= (n + 135) / 136: an emitted frame owns two flags and 120 bits); the carried
 *                                                      state is the raw bytes of the open frame (at most 3185 + 7) or the last 7 bytes; bit-identical
 *                                                      however the stream is cut.  Fuses with nothing.
 *   "pocsagframer"                                     (pocsagframer.lua:120-277; no parameters, any is refused) Bit -> little-endian records, the tail
 *                                                      of `data` behind `count` zero:
 *                                                        struct lrhip_pocsag_frame {    256 bytes: one dword per lane of a wave
 *                                                          uint32_t address;            21 bits
 *                                                          uint8_t func;                2 bits
 *                                                          uint8_t flags;               bit 0: this frame continues in the next record;
 *                                                                                       bit 1: this record continues the previous one
 *                                                          uint16_t count;              data words in this record, 0 .. 62
 *                                                          uint32_t data[62]; };        20-bit data words
 *                                                      The reference's frame has no upper length: a frame of more than 62 data words is a chain of
 *                                                      records, a full one written with bit 0 set when the 63rd word arrives, its successor with bit 1
 *                                                      and the same address and func.  Nothing is dropped.  FRAME_SYNC: the first position whose 32
 *                                                      bytes correlate with the sync word, sum(s_i (2 value_i - 1)) >= 28 on the byte values.  BATCH,
 *                                                      once 544 bytes are there: codeword 0 (a byte is a 1 only when it equals 1) must correct - zero or
 *                                                      single-bit-error syndrome - to 0x7cd215d8, else the pending frame goes out, 32 bytes are
 *                                                      consumed and the search resumes; then 16 codewords: uncorrectable, idle and address codewords
 *                                                      emit the pending frame, an address codeword opens one, a data codeword appends to an open one,
 *                                                      two uncorrectable in a row at position j consume (j + 1) 32 bytes and resume the search.
 *                                                      TIMING: the reference takes one step per loop iteration after refilling its buffer, so it stops
 *                                                      with up to 543 buffered bits unexamined and its output depends on how the stream was cut.  The
 *                                                      stage is EAGER: it takes every step the bits seen so far allow (32 or more in FRAME_SYNC, 544 in
 *                                                      BATCH).  Its output is the same however the stream is cut; whatever the reference emits for any
 *                                                      cutting is a prefix of it; and it is a prefix of the reference's output once 544 further bits
 *                                                      have been fed.  Count data-dependent (<= (n + 543) / 32: a record goes with 32 consumed
 *                                                      bytes); the carried state is the pending frame and the at most 543 unconsumed bytes; reset
 *                                                      drops both.  Fuses with nothing.
 *   "pam:period=P:bits=b:msb=0|1:table=a0,a1,..."     (pulseamplitudemodulator.lua:57-87) Bit -> Float32: b bits (a byte counts as 1 only when it equals
 *                                                      1; msb=1: the first bit is the most significant) select one of the 2^b table entries, which is
 *                                                      held for P output samples.  P = floor(sample_rate / symbol_rate) in 1 .. 2^30 - 1, b in 1 .. 16,
 *                                                      integers; the table as decimal (%.9g) or hexadecimal floating-point text, read with strtod and
 *                                                      rounded to Float32 (both forms give back the Float32 they were printed from).  A call emits
 *                                                      floor((pending + n) / b) P samples (max_output: ceil(n / b) P) and carries the remaining < b bits;
 *                                                      no read-back.  rate() = b : P, memory() = 0; lrhip_stage_seek(n0) needs n0 % b == 0 (the bits another
 *                                                      partition holds back are unknown) and fails otherwise, leaving the stage as it was.
 *   "qam:period=P:bits=b:msb=0|1:table=re0,im0,re1,im1,..."  (quadratureamplitudemodulator.lua:69-99) Bit -> ComplexFloat32, otherwise as "pam".
 *   "pamdemod:period=P:offset=o:bits=b:msb=0|1:soft=0|1:weight=w:grid=1:table=a0,a1,..."  (no block of the reference: the inverse of "pam") Float32 ->
 *                                                      Bit, or -> Float32 with soft=1.  Symbol s of the stream is decided on input sample s P + offset
 *                                                      (o in 0 .. P - 1) against the 2^b table entries, which the caller has already scaled to the received
 *                                                      amplitudes.  Float32 arithmetic, each operation rounded on its own: d_v = fl(dr dr), dr = x - a_v.
 *                                                      Hard: the first v with the smallest d_v (best = +inf, v taken when d_v < best; a NaN or infinite sample
 *                                                      decides 0), written as b Bit bytes, positions b-1 .. 0 of v with msb=1, else 0 .. b-1.  Soft: in the same
 *                                                      order llr_k = fl(fl(m1_k - m0_k) w), m0_k / m1_k the smallest d_v over the entries with bit k clear / set
 *                                                      (the same comparison from +inf), w a finite Float32 above 0; positive = bit 0.  All keys are required;
 *                                                      P, b and the table's text as "pam".  The only state is the absolute input position: a call emits b
 *                                                      outputs per symbol whose sample it delivers (max_output: (n / P + 1) b; possibly none), no read-back,
 *                                                      any chunking gives the same bytes; lrhip_stage_seek(n0) takes any n0 and continues at symbol
 *                                                      ceil((n0 - o) / P) (0 while n0 <= o).  rate() = P : b, memory() = 0.  Fuses with nothing.
 *   "qamdemod:period=P:offset=o:bits=b:msb=0|1:soft=0|1:weight=w:grid=qb|-1:table=re0,im0,re1,im1,..."  ComplexFloat32 -> Bit / Float32, as "pamdemod"
 *                                                      with d_v = fl(fl(dr dr) + fl(di di)).  grid=-1: the search over all entries, b <= 12.  grid=qb, 0 <= qb <= b:
 *                                                      the caller states that table[v] = (I[v >> qb], Q[v & (2^qb - 1)]) bit for bit for every v (checked; b <= 16)
 *                                                      and each axis is decided on its own by the same rule on fl(dr dr) and fl(di di), the two indices joined:
 *                                                      differs from grid=-1 only where two candidates differ before the final addition and coincide after it, or
 *                                                      one component is NaN.  Soft output is the same Float32 in both forms (m = fl(min_i a_i + min_q b_q) with
 *                                                      the bit's axis restricted to its half).
 *   "pfbsynthesizer:channels=K:oversample=R:taps=g0,g1,..."  (no block of the reference: the inverse of lrhip_pfb_oversampled_create) the K-channel synthesis
 *                                                      filterbank in its polyphase + FFT form: K chains Upsampler(D) -> FIR(g) -> FrequencyTranslator(+c / K),
 *                                                      D = K / R, summed, with zero history:  xhat[n] = sum_c exp(+j 2 pi c n / K) sum_m g[n - m D] Y[m, c].
 *                                                      ComplexFloat32 -> ComplexFloat32.  The input is the frame stream the analysis bank emits (K values per
 *                                                      frame, channel c at position c) and n_in counts VALUES: a call may end inside a frame, whose values
 *                                                      are carried; a call emits D samples per frame it completes (max_output: ceil(n / K) D).  The domain
 *                                                      is the analysis bank's: K a power of two in [8, 4096], K <= #taps <= min(64 K, 65536), R in {1, 2, 4};
 *                                                      the taps as the "pam" table (%.9g or hexadecimal floating-point text).  Every output is one fmaf chain
 *                                                      over the Q = ceil(#taps / D) frames under its taps, oldest first, so any chunking gives the same
 *                                                      bytes; a non-finite value in frame m makes exactly outputs m D .. m D + #taps - 1 non-finite.
 *                                                      Carried: the partial frame, the transformed last Q - 1 frames, the frame count modulo R; reset drops
 *                                                      all three.  rate() = R : 1, memory() = -1, seek is refused.  Fuses with nothing.
 *   "signalsource:signal=exponential|cosine|sine|square|triangle|sawtooth|constant:frequency=F:rate=R:amplitude=A:phase=P:offset=O"
 *                                                      (sources/signal.lua) a SOURCE: no input, lrhip_stage_input_size() = 0; ComplexFloat32 for
 *                                                      exponential, Float32 otherwise.  Every key once; doubles as %.17g text, finite, R > 0.  Sample n
 *                                                      is a closed form of the absolute index: turns(n) = p0 + n step in wrapping uint64 arithmetic,
 *                                                      with fx(x) = uint64(rint(ldexp(x - floor(x), 64))) mod 2^64, step = fx(F / R),
 *                                                      p0 = fx(P / 6.283185307179586).  exponential: A (c, s), the translator's phasor of turns(n), O
 *                                                      ignored; cosine: c A + O; sine: s A + O; with td = (turns >> 11) 2^-53 and first = turns < 2^63,
 *                                                      square: w = first ? 1 : -1, triangle: w = first ? 1 - 4 td : 4 td - 3, sawtooth: w = 2 td - 1,
 *                                                      the sample w A + O; constant: A alone.  One double multiply and one double add, rounded once
 *                                                      to Float32.  The reference adds omega to a running double phase, wraps it once per 8192-sample
 *                                                      chunk and takes cosf / sinf of the phase rounded to Float32: its own output is off the exact
 *                                                      waveform by up to A ulp_f32(2 pi + 8192 omega) / 2 (signal_spec.lua's 2e-5 epsilon), and it
 *                                                      cannot be cut or sought.  Here any chunking gives the same bits, lrhip_stage_seek(n0) sets the
 *                                                      index, reset puts it back to 0, memory() = 0, rate 1 : 1, max_output(n) = n.
 *   "uniformrandomsource:type=cf32|f32|byte|bit:lo=L:hi=H:seed=S"
 *                                                      (sources/uniformrandom.lua) a SOURCE of ComplexFloat32, Float32, Byte or Bit samples; L <= H
 *                                                      finite doubles (Byte: integers in 0 .. 255; Bit: ignored), S a decimal uint64.  Word j of the
 *                                                      stream is output j & 3 of Philox4x32-10 with counter (lo32(j >> 2), hi32(j >> 2), 0, 0) and key
 *                                                      (lo32(S), hi32(S)); u(j) = w(j) 2^-32.  f32: float(L + (H - L) u(n)) in double, not contracted;
 *                                                      cf32: re from w(2 n), im from w(2 n + 1); byte: L + ((w(n) (H - L + 1)) >> 32); bit: w(n) >> 31.
 *                                                      The reference draws from LuaJIT's sequential math.random, whose values nobody relies on: the
 *                                                      contract is distribution, range and determinism per seed.  Chunking, seek, reset, memory() as
 *                                                      the signal source.
 *   "arbresampler:type=cf32|f32:phases=P:step=S:taps=h0,h1,..."
 *                                                      (no block of the reference) a resampler for any rate ratio in [1/16, 16]: a bank of P phases
 *                                                      (a power of two, 16 .. 256), linearly interpolated between neighbouring phases.  S, a decimal
 *                                                      uint64 in [2^44, 2^52], is the input samples per output sample in 16.48 fixed point
 *                                                      (rint(2^48 / ratio)); the taps are a prototype of P T Float32 values at P times the input
 *                                                      rate, T = 4 .. 512 per phase, P T <= 8192.  G[p][k] = h[k P + p], row P = row 0 one tap later,
 *                                                      D[p][k] = float(G[p + 1][k] - G[p][k]).  Absolute output m: u = m S (128 bits), i = u >> 48,
 *                                                      f = u mod 2^48, p = f >> (48 - log2 P), mu = ((f >> (24 - log2 P)) mod 2^24) 2^-24, and
 *                                                      y[m] = sum_k fmaf(mu, D[p][k], G[p][k]) x[i - k], one fmaf chain per component in ascending k,
 *                                                      x[j] = 0 for j < 0.  Output m is emitted once input i has arrived: after Q inputs in all
 *                                                      ceil(Q 2^48 / S) outputs exist, a call returns what is new (possibly 0 samples).  Any chunking
 *                                                      gives the same bits; max_output(n) = floor(n 2^48 / S) + 2, rate() = S : 2^48 in lowest terms,
 *                                                      memory() = T - 1, lrhip_stage_seek(n0) continues at output ceil(n0 2^48 / S).  The domain is
 *                                                      checked before the device is looked at; the stage fuses with nothing.
 *   "convenc:k=K:polys=g0,g1,..."                      (no block of the reference) Bit -> Bit, a rate-1/n convolutional encoder: K = 3 .. 9, n = 2 .. 4
 *                                                      polynomials as OCTAL text ("polys=171,133"), each below 2^K, bit K - 1 multiplying the current
 *                                                      input bit; at least one polynomial has bit K - 1 and one has bit 0.  r = (u << (K - 1)) | (r >> 1)
 *                                                      from r = 0 at bit 0 of the stream (bit 0 of each input byte is read), out[n t + j] =
 *                                                      parity(r & g_j).  max_output(m) = n m, rate() = 1 : n, memory() = K - 1, lrhip_stage_seek(n0)
 *                                                      takes any n0 and continues at output n n0.
 *   "viterbi:k=K:polys=g0,g1,...:input=llr|bit:scale=s:block=D:depth=L"
 *                                                      (no block of the reference) the windowed Viterbi decoder of that code.  input=llr: Float32 LLRs,
 *                                                      positive = 0, each quantised once to q = clamp(rintf(float(llr s)), -127, 127), NaN -> 0;
 *                                                      input=bit: q = 127 (1 - 2 b).  s a finite Float32 above 0, D = 64 .. 2048, L = K - 1 .. 256,
 *                                                      (D + 2 L) 2^(K - 1) / 8 <= 65536.  All keys are required.  Step t reads the inputs n t .. n t + n - 1
 *                                                      of the stream; window w decodes the bits [w D, (w + 1) D) from the steps max(0, w D - L) ..
 *                                                      (w + 1) D + L - 1 in int32 (csrc/kernels_viterbi.h has the trellis and the tie rules), starting
 *                                                      from state 0 at step 0 and from equal metrics elsewhere, and tracing back from the best final
 *                                                      state.  After Q inputs, E = floor(Q / n), floor((E - L) / D) windows are out (none while E < L):
 *                                                      a call returns the windows it completes, possibly none, from the lengths alone.  There is no
 *                                                      flush: the last fewer than D + L bits of a stream never leave.  Any chunking gives the same
 *                                                      bytes; max_output(N) = D ceil(ceil(N / n) / D), rate() = n : 1, memory() = n (D + 2 L) - 1;
 *                                                      lrhip_stage_seek(n0) takes any n0, continues at bit D floor((floor(n0 / n) - L) / D) and counts the
 *                                                      inputs in front of n0 as erasures.  Both stages check their domain before the device is
 *                                                      looked at and fuse with nothing.
 *   "rsenc:n=N:k=K:gfpoly=P:fcr=F:prim=R:interleave=I" (no block of the reference) Byte -> Byte, a systematic Reed-Solomon encoder over GF(2^8) in the
 *                                                      polynomial basis.  All keys are required and DECIMAL: gfpoly=285 is 0x11d.  gfpoly is one of
 *                                                      the 16 primitive polynomials of degree 8 (alpha = 2 must have order 255), fcr = 0 .. 254,
 *                                                      prim = 1 .. 254 coprime to 255: g(x) = prod_{i < N - K} (x - alpha^((fcr + i) prim)).
 *                                                      3 <= N <= 255, K >= 1, N - K even and 2 .. 64; N < 255 is the shortened code (255 - N virtual
 *                                                      zeros at the highest degrees).  Byte j of a codeword is the coefficient of x^(N - 1 - j): the K
 *                                                      message bytes, then N - K parity bytes.  I = 1 .. 8 codewords are symbol-interleaved: a frame
 *                                                      is I K bytes in and I N bytes out, byte j of a frame belongs to codeword j mod I at index
 *                                                      j div I, the output frame is the I K message bytes as they came, then the parity bytes
 *                                                      interleaved the same way.
 *   "rsdec:n=N:...:interleave=I:status=0|1"            (no block of the reference) its bounded-distance decoder, the same keys and status.  A frame is
 *                                                      I N bytes in and the I K corrected message bytes out, followed with status=1 by I status bytes,
 *                                                      one per codeword: the symbols corrected, 0 .. t = (N - K) / 2 (parity bytes count), or 255 for
 *                                                      an uncorrectable word, whose message bytes leave as received (Berlekamp-Massey register longer
 *                                                      than t, not exactly that many locator roots among the N real positions, or a zero error
 *                                                      magnitude).  No erasure input.
 *   "packbits:order=msb|lsb"                           (no block of the reference) Bit -> Byte, eight bits (bit 0 of each input byte) per byte on
 *                                                      absolute bit indices, frames of 8 in and 1 out; msb: the first bit is the most significant.
 *   "unpackbits:order=msb|lsb"                         (no block of the reference) Byte -> Bit, frames of 1 in and 8 out.
 *                                                      These four are stages of whole frames, FI bytes in and FO bytes out: frame f is the input bytes
 *                                                      [f FI, (f + 1) FI) of the stream, a call returns the frames its input completes, possibly none,
 *                                                      from the lengths alone, and there is no flush.  Any chunking gives the same bytes;
 *                                                      max_output(N) = FO ceil(N / FI), rate() = FI : FO in lowest terms, memory() = FI - 1;
 *                                                      lrhip_stage_seek(n0) takes any n0 whose output position is below 2^64, continues at output
 *                                                      FO floor(n0 / FI) and counts the bytes of that frame in front of n0 as zeros.  They check
 *                                                      their domain before the device is looked at and fuse with nothing.
 *   "puncture:pattern=B"                               (no block of the reference) Bit -> Bit.  B is 2 .. 64 characters 0 / 1, not all 0: a stage of
 *                                                      whole frames as the four above, counted in elements, len(B) in and popcount(B) out, element j
 *                                                      of a frame kept where B[j] is 1.  Bytes are moved, never interpreted.
 *   "depuncture:pattern=B:input=llr|bit"               (no block of the reference) the inverse framing, Float32 (llr) or Bit (bit) -> Float32:
 *                                                      popcount(B) elements in, len(B) Float32 out, +0.0f - an erasure to "viterbi" - where B[j] is 0.
 *                                                      llr: the four bytes of an input are moved as they are (a NaN stays that NaN); bit: bit 0 of the
 *                                                      byte is read, 0 gives +1.0f and 1 gives -1.0f, which "viterbi" at scale=127 reads as its hard
 *                                                      input.  Contract of the frame stages, with elements for bytes.
 *   "convinterleave:branches=I:step=M"                 (no block of the reference) Byte -> Byte, 1 : 1, the convolutional (Forney) interleaver:
 *                                                      I = 2 .. 256, M = 1 .. 256, depth D = (I - 1) M I <= 65536.  With j = i mod I on the absolute
 *                                                      index i, out[i] = in[i - j M I] and in[negative] = 0.
 *   "convdeinterleave:branches=I:step=M"               its inverse up to a delay of D bytes: out[i] = in[i - (I - 1 - j) M I].  Both carry the last D
 *                                                      input bytes between calls; max_output(n) = n, memory() = D, lrhip_stage_seek(n0) takes any n0
 *                                                      and continues at output n0 with zeros for everything in front.
 *   "scrambler:table=HEX:offset=K"                     (no block of the reference) Byte -> Byte, 1 : 1, additive: HEX is 2 P hexadecimal digits, the
 *                                                      P = 1 .. 8192 bytes of the table, K = 0 .. P - 1; out[i] = in[i] ^ table[(i + K) mod P] on the
 *                                                      absolute index i (reduced mod P before K is added: no i below 2^64 wraps).  memory() = 0,
 *                                                      lrhip_stage_seek(n0) takes any n0.  The library knows no polynomial: the caller builds tables.
 *                                                      All keys of these five are required; they check their domain before the device is looked at
 *                                                      and fuse with nothing.
 *   "pll:alpha=A:beta=B:fmin=F0:fmax=F1:mult=M:port=out|error"
 *                                                      PLLBlock, ComplexFloat32 -> ComplexFloat32 cis(phi_multiplied) (port=out, the default) or
 *                                                      Float32 phase error (port=error).  A, B, F0, F1 (radians per sample) are required and finite,
 *                                                      M defaults to 1.  While the loop is in lock a call is computed in parallel segments whose
 *                                                      speculated entry states are verified against their predecessors' exits, and rejected segments
 *                                                      are rerun serially (csrc/pll_plan.h).  The result is the reference's serial recurrence with
 *                                                      perturbations at accepted segment boundaries of at most 2^-22 rad in phi_locked (modulo 2 pi)
 *                                                      and 2^-22 B / A in freq_locked.  These tolerances bound phi_locked and freq_locked, and with
 *                                                      them the error port; they do NOT bound phi_multiplied, which is never fed back: each accepted
 *                                                      boundary can move it by up to (|M| + |M - 1|) 2^-22 rad, so the out port's distance from the
 *                                                      serial loop grows with the stream length and the multiplier (measured on the host at M = 20,
 *                                                      carrier + 0.1 noise, segments of 64: 4e-7 after 2^15 samples, 8e-7 after 2^16 and rising; at
 *                                                      M = 3 it stays at Float32 rounding).  Segments whose mean |error| is under 1e-5 rad (a tone
 *                                                      without noise) or over pi / 4 (no lock) are always rerun serially.  The test knob
 *                                                      "speculate=0" runs the serial recurrence throughout and gives its value at any length.
 *                                                      memory() = -1: no time partitions.  The stage fuses with nothing.
 * A source runs with in = NULL and n_in = the number of samples to generate, in every execute / submit entry point; a chain takes one as its
 * first stage only.
 * The sampler, the clocksampler, the preamblesampler, the manchesterdecoder, the varicodedecoder, the rdsframer, the three ERT framers, the ax25framer and the pocsagframer have memory() -1: chains holding them refuse time
 * partitions. */
lrhip_stage_t *lrhip_unary_create(const char *op, float re, float im, int constant_complex, int input_complex);

/* Port tables: the many-ported stages.  Four ops of lrhip_unary_create (re / im / constant_complex / input_complex ignored) make stages
 * with N input ports or N output ports; they are stateless, memory() = 0, and fuse with nothing:
 *   "interleave:channels=N:size=4|8"      (interleave.lua:47-58) N inputs of 4- or 8-byte samples -> out[N i + k] = in_k[i]; bytes are moved,
 *                                         never interpreted.  max_output(n) = N n; returns N n.
 *   "deinterleave:channels=N:size=4|8"    (deinterleave.lua:49-63 with index = 0) one input -> out_j[i] = in[N i + j]: port j receives
 *                                         ceil((n - j) / N) samples, n need be no multiple of N.  max_output(n) = ceil(n / N); returns port 0's
 *                                         count.  The reference's carried index is the caller's: it rotates the table (entry j = the channel of
 *                                         this call's j-th sample).
 *   "wavpack:channels=N:bits=8|16|32"     (sinks/wavfile.lua:171-176) N Float32 inputs -> records of N raw samples (u8 / s16le / s32le),
 *                                         raw[N i + k] = pack(in_k[i]) with the arithmetic and the saturation rule of lrhip_format_pack_create.
 *                                         output_size = N bits / 8; returns n records.
 *   "wavunpack:channels=N:bits=8|16|32"   (sources/wavfile.lua:235-239) n whole records (input_size = N bits / 8) -> N Float32 outputs,
 *                                         out_k[i] = (raw[N i + k] - offset) / scale as lrhip_format_convert_create; returns n.
 * channels: an integer, 2 .. 32 (the WAV pair: 1 .. 32); anything else is refused at creation.
 *
 * They run through lrhip_stage_execute_device alone, and the many-ported side of the call is a PORT TABLE, a small structure in HOST memory:
 *
 *     { uint32_t magic;            0x5450524c, the bytes "LRPT"
 *       uint32_t count;            the stage's channel count
 *       void    *ptr[count]; }     ptr[k]: the DEVICE address of port k
 *
 *   N-input stage  (interleave, wavpack):      in_dev  = the address of the table, n_in = samples per port; out_dev a device vector.
 *   N-output stage (deinterleave, wavunpack):  out_dev = the address of the table, out_capacity = the capacity of EACH port; in_dev a device vector.
 *
 * The library reads the table on the host before anything is launched and refuses, with its own lrhip_strerror() message, a wrong magic, a
 * count other than the stage's channels and a null pointer.  The pointers travel to the kernel by value in its argument block: nothing is
 * copied to the device, no device-side table exists, and the table may be freed as soon as the call returns.  Ports may have any alignment;
 * a port that is 16-byte aligned is moved 16 bytes per lane.  lrhip_stage_execute (host buffers), lrhip_stage_execute2* and
 * lrhip_chain_create* refuse these stages.  (The table is a documented layout, not a declared type: luaradio_amd/_lib.py port_table() builds it.) */
/* DelayBlock (radio/blocks/signal/delay.lua:26-72): delay by num_samples (> 0), zero initial state. elem_size 8 or 4. */
lrhip_stage_t *lrhip_delay_create(unsigned num_samples, int elem_size);
/* HilbertTransformBlock (radio/blocks/signal/hilberttransform.lua:25-37, :100-160): Float32 in, ComplexFloat32 out =
 * (input delayed by (M-1)/2, input filtered by the M Hilbert taps).  taps: M (odd) floats from fir_hilbert_transform. */
lrhip_stage_t *lrhip_hilbert_create(const float *taps, unsigned ntaps);

/* Welch / Bartlett averaged power spectrum, the arithmetic of GnuplotSpectrumSink / GnuplotWaterfallSink
 * (radio/blocks/sinks/gnuplotspectrum.lua:140-186): frames of n samples every (n - overlap) samples, each frame's PSD
 * (arguments as lrhip_psd_create, spectrum fftshifted) accumulated on the device.  The stage is a sink:
 * lrhip_stage_execute*() consumes the chunk and returns 0 outputs; partial frames are carried to the next call.
 * lrhip_welch_read() writes the n-point average (sum / frames) to avg_host and returns the number of frames averaged
 * (0: nothing accumulated, avg_host untouched); reset != 0 clears the accumulator (gnuplotspectrum.lua:189-191). */
lrhip_stage_t *lrhip_welch_create(unsigned n, const float *window, double scale, int logarithmic, int input_complex, unsigned overlap);
long lrhip_welch_read(lrhip_stage_t *q, float *avg_host, int reset);

/* Critically sampled K-channel analysis filterbank (BASELINE.json configs[4]; not a block of the reference: defined as
 * K parallel chains FrequencyTranslatorBlock(-c*fs/K) -> FIRFilterBlock(taps) -> DownsamplerBlock(K), c = 0..K-1).
 * ComplexFloat32 in; one output frame of K ComplexFloat32 values (channel-major within the frame) per K input
 * samples, with the downsampler's carried index.  Computed as one dense GEMM on the f32 matrix cores.
 * nchannels in {32, 64}; ntaps a multiple of 32. */
lrhip_stage_t *lrhip_channelizer_create(const float *taps, unsigned ntaps, unsigned nchannels);

/* The same filterbank (same frames, same emission rule and carried index) in its polyphase + FFT form: P = ceil(ntaps / nchannels)
 * real-by-complex multiply-adds per sample and one inverse DFT of nchannels points per frame, instead of the GEMM's 8 * ntaps flop
 * per sample.  nchannels a power of two in [8, 4096]; nchannels <= ntaps <= min(64 * nchannels, 65536), any value in between. */
lrhip_stage_t *lrhip_pfb_channelizer_create(const float *taps, unsigned ntaps, unsigned nchannels);

/* The polyphase + FFT filterbank oversampled by R = oversample in {1, 2, 4}: K parallel chains FrequencyTranslatorBlock(-c*fs/K) ->
 * FIRFilterBlock(taps) -> DownsamplerBlock(D), D = nchannels / R, so that a prototype whose skirt reaches past fs / (2 K) no longer aliases
 * into its channel.  One frame of K values per D input samples (frame m as soon as sample m D has arrived), each channel at R fs / K:
 *     y_c[m] = exp(-j 2 pi c m D / K) * sum_{i<ntaps} taps[i] * x[m D - i] * exp(+j 2 pi c i / K)
 * Frame m R is frame m of the critically sampled bank.  Same domain as lrhip_pfb_channelizer_create (nchannels = 8 with R = 4 included);
 * oversample = 1 is that stage.  The carried state is the index, the last ntaps - 1 samples and the frame count modulo R.
 * max_output(n) = (n / D + 1) * K. */
lrhip_stage_t *lrhip_pfb_oversampled_create(const float *taps, unsigned ntaps, unsigned nchannels, unsigned oversample);

void lrhip_stage_destroy(lrhip_stage_t *q);
/* Back to the just-created state (zero history, phase 0, index 0). */
int lrhip_stage_reset(lrhip_stage_t *q);
/* Bytes per input / output sample (8 or 4; 1 for Bit / Byte streams, the record size for raw records and frames; input 0: a source). */
int lrhip_stage_input_size(const lrhip_stage_t *q);
int lrhip_stage_output_size(const lrhip_stage_t *q);
/* Upper bound on the samples execute() will write for n_in inputs, so the caller can
 * `self.out:resize()` first (firfilter.lua:130). */
unsigned long lrhip_stage_max_output(const lrhip_stage_t *q, unsigned long n_in);

/* ---- execution --------------------------------------------------------------------------------------- */
/* One block's process() with host buffers: H2D through a pinned ring, kernels, D2H, wait.
 * Returns the number of output samples written, or < 0. */
long lrhip_stage_execute(lrhip_stage_t *q, const void *in_host, unsigned long n_in,
                         void *out_host, unsigned long out_capacity);
/* Same, with device pointers, asynchronous on the library stream (no copies, no wait).  The output count is
 * known on the host without a device round-trip.  This is what chains and bench.py use.
 * Exception: a stage whose output count depends on the data (the sampler, the clocksampler) reads its count word back and waits for its
 * own kernels; so does a chain holding one (lrhip_chain_execute_device, and lrhip_chain_submit, whose return value is then the exact count). */
long lrhip_stage_execute_device(lrhip_stage_t *q, const void *in_dev, unsigned long n_in,
                                void *out_dev, unsigned long out_capacity);

/* Two-input variants for lrhip_binary_create() stages (both inputs n_in samples). */
long lrhip_stage_execute2(lrhip_stage_t *q, const void *in1_host, const void *in2_host, unsigned long n_in,
                          void *out_host, unsigned long out_capacity);
long lrhip_stage_execute2_device(lrhip_stage_t *q, const void *in1_dev, const void *in2_dev, unsigned long n_in,
                                 void *out_dev, unsigned long out_capacity);

/* ---- chains: several blocks, device-resident edges ------------------------------------------------------ */
/* A maximal linear run of device-capable blocks collapsed into one object (what CompositeBlock's
 * _prepare_to_run would build, radio/core/composite.lua:426): one H2D at the head, one D2H at the tail,
 * intermediate vectors never leave HBM.  The chain borrows the stages (caller keeps ownership) and fuses
 * adjacent stages where a fused kernel exists (rotator -> FIR -> downsampler, FIR -> downsampler, ... -> discriminator, the 1/5-rate
 * audio tail of the FM receivers).  A chain gives the values of its blocks run one by one - the same bits, with FIVE stated exceptions
 * (each a different rounding of the same mathematics, none above 1e-6 of the exact result):
 *   1. overlap-save filters (Float32 FFT arithmetic: the blocks of a chunk fall where the chunk starts, <= 1e-6);
 *   2. the polyphase audio tail (FIR -> single-pole IIR -> downsampler as one decimating filter, ~2e-8 RMS);
 *   3. a frequency translator fused in front of a filter whose output only the discriminator sees: a tile's window is rotated relative to
 *      its first sample, which leaves the angles unchanged to Float32 rounding of the filter outputs;
 *   4. the FM receiver in ONE launch (kernels_rx.h; the default for the tuner + discriminator + audio-tail shape of
 *      examples/rtlsdr_wbfm_mono.lua:12-17 whose de-emphasis pole q at the audio rate satisfies q^75 <= 2^-25): the recurrence of every
 *      workgroup run restarts from a zero state 75 audio samples early and the runs fall with the chunk length, so the audio depends on
 *      the chunking and on the grid to <= 2e-7 (tests/test_gpu_rx.py), and time partitions agree with the single stream to 1e-7
 *      rather than bit for bit;
 *   5. consecutive overlap-save filters on a ComplexFloat32 stream merged into ONE filter with the taps convolved in double (up to 1 281
 *      taps): rounds once where the cascade rounds per stage, <= 1e-6 of the exact cascade.
 * lrhip_chain_create_ex() below switches 2-5 off per chain (LRHIP_CHAIN_EXACT); 1 is chosen per filter (use_fft = 0: direct form).
 *
 * A SOURCE (lrhip_stage_input_size() = 0: "signalsource", "uniformrandomsource") may be the FIRST stage of a chain, nowhere else.  Such a chain has no input:
 * lrhip_chain_execute, _execute_device and lrhip_chain_submit take in = NULL and n_in = the number of samples to generate, and copy nothing to the device;
 * the source runs as a launch of its own (it fuses with nothing).  The ring (set_ring / submit / collect), seek, halo, shard_align and start_at work as
 * for any chain - the input samples start_at drops are the generated ones.  The entry points that move input bytes - lrhip_chain_push,
 * lrhip_chain_ring_input, lrhip_chain_submit_fd - refuse it with a message. */
lrhip_chain_t *lrhip_chain_create(lrhip_stage_t **stages, unsigned nstages);
/* The numerical contract per chain (what a LuaRadio script sets as DeviceChainBlock.exact, lua/radio/composites/devicechain.lua).
 * lrhip_chain_create(stages, n) == lrhip_chain_create_ex(stages, n, 0).  Flags:
 *   LRHIP_CHAIN_EXACT_ROTATOR      a frequency translator fused in front of a filter keeps the stand-alone translator's phasors
 *                                  (block-of-8 staging): fused == unfused and chunked == unchunked bit for bit, at 0.19 instead of
 *                                  0.16 ms per 2^26 samples of the WBFM receiver;
 *   LRHIP_CHAIN_NO_POLYPHASE_TAIL  FIR -> single-pole IIR -> downsampler keeps the blocks' own arithmetic (filter at the high rate,
 *                                  recurrence, gather) instead of ONE decimating filter with the recurrence at the low rate; and
 *                                  consecutive overlap-save filters on a ComplexFloat32 stream stay separate filters instead of ONE
 *                                  filter with the convolved taps (up to 1 281 taps, one 4096-point launch);
 *   LRHIP_CHAIN_NO_FUSION          every stage runs its own kernels (edges still device-resident);
 *   LRHIP_CHAIN_NO_SINGLE_LAUNCH   the FM receivers keep tuner + discriminator and audio tail as two launches (the round-2 form).
 * LRHIP_CHAIN_EXACT = EXACT_ROTATOR | NO_POLYPHASE_TAIL | NO_SINGLE_LAUNCH: the chain computes what its blocks compute one by one (bit for bit
 * for direct-form filters; overlap-save filters stay within 1e-6, as in the reference).  The environment variables LRHIP_TUNER_EXACT,
 * LRHIP_NO_POLYPHASE_TAIL, ... of DESIGN.md 4.5 remain as process-wide overrides for A/B measurements.  Unknown bits -> NULL. */
enum {
    LRHIP_CHAIN_EXACT_ROTATOR = 1,
    LRHIP_CHAIN_NO_POLYPHASE_TAIL = 2,
    LRHIP_CHAIN_NO_FUSION = 4,
    LRHIP_CHAIN_NO_SINGLE_LAUNCH = 8,
    LRHIP_CHAIN_EXACT = 1 | 2 | 8
};
lrhip_chain_t *lrhip_chain_create_ex(lrhip_stage_t **stages, unsigned nstages, unsigned flags);
void lrhip_chain_destroy(lrhip_chain_t *c);
/* Back to the initial state (zero history, phase, indices) for every stage of the chain, including the fused ones it built. */
int   lrhip_chain_reset(lrhip_chain_t *c);
unsigned long lrhip_chain_max_output(const lrhip_chain_t *c, unsigned long n_in);
long lrhip_chain_execute(lrhip_chain_t *c, const void *in_host, unsigned long n_in,
                         void *out_host, unsigned long out_capacity);
long lrhip_chain_execute_device(lrhip_chain_t *c, const void *in_dev, unsigned long n_in,
                                void *out_dev, unsigned long out_capacity);
/* Pipelined host path: the chain owns a RING of `depth` slots, each a pinned host input/output buffer plus device
 * input/output buffers sized for `max_chunk` input samples.  submit() copies the caller's vector into the next
 * pinned slot and enqueues H2D (copy-in stream) -> the chain's kernels (compute stream) -> D2H (copy-out stream),
 * chained by events, and returns at once; collect() waits for the OLDEST submitted chunk and hands back its output.
 * With depth >= 2 the PCIe transfers of neighbouring chunks overlap the kernels, and the block's process() can return
 * chunk k-depth+1 while chunk k is in flight (the reference's own FFT FIR also delays its output, firfilter.lua:361-398).
 * Block state is advanced at submit time, so results are identical to lrhip_chain_execute() chunk for chunk.
 * submit() returns the number of output samples the chunk WILL produce (>= 0) or < 0; collect() returns the number of
 * samples written, or < 0 (-2: nothing in flight).  This is what radio/core/pipe.lua's read/write loop
 * (pipe.lua:495-533, :252-262) becomes for a device chain. */
int  lrhip_chain_set_ring(lrhip_chain_t *c, unsigned depth, unsigned long max_chunk);
long lrhip_chain_submit(lrhip_chain_t *c, const void *in_host, unsigned long n_in);
/* Zero-copy input: the pinned host buffer of the slot the NEXT lrhip_chain_submit() will use (max_chunk input samples), or
 * NULL when the ring is full.  A source can read()/recv() straight into it and pass the same pointer to
 * lrhip_chain_submit(), which then skips its staging copy. */
void *lrhip_chain_ring_input(lrhip_chain_t *c);
/* File-fed chains: what IQFileSource / RealFileSource do per chunk (radio/blocks/sources/iqfile.lua:82-96: fread of raw records) without the interpreter or a
 * staging copy in the data path.  Reads up to max_in samples - raw records of lrhip_stage_input_size(first stage) bytes, max_in clamped to the ring's max_chunk -
 * of the REGULAR file `fd` from byte offset `offset` (positional reads: the descriptor's own position is neither used nor moved) straight into the pinned input of
 * the next ring slot, split over the library's copy threads (one read(2) stream gets ~10 GB/s out of the page cache, several get several times that), and submits
 * the slot as lrhip_chain_submit() does.  Returns the number of samples read and submitted; 0 at the end of the file (nothing submitted; a trailing partial
 * record is ignored, as fread() ignores it); < 0 on error: -3 ring full (collect first), -4 `fd` is not a regular file (pipes, sockets, devices: read() into
 * lrhip_chain_ring_input() and call lrhip_chain_submit()). */
long lrhip_chain_submit_fd(lrhip_chain_t *c, int fd, unsigned long long offset, unsigned long max_in);
long lrhip_chain_collect(lrhip_chain_t *c, void *out_host, unsigned long out_capacity);
/* Chunks submitted and not yet collected. */
int  lrhip_chain_in_flight(const lrhip_chain_t *c);
/* Chunk coalescing on top of the ring (what a DeviceChainBlock's process() calls): LuaRadio hands blocks whatever a read() returned,
 * 8 192 samples from a file source (radio/blocks/sources/iqfile.lua:52), up to 131 072 from a pipe (radio/core/pipe.lua:495-533) -
 * far too little for one launch set.  push() appends the caller's vector to the pinned input of the current ring slot and returns at
 * once; a slot is launched (H2D, kernels, D2H, asynchronously as for submit()) when it holds max_chunk samples, and the outputs of
 * slots that have finished are copied to out_host in stream order.  Sample VALUES are those of lrhip_chain_execute() on the same
 * stream (block state does not depend on chunking); only the emission is delayed, as the reference's own FFT filter delays its
 * output (firfilter.lua:361-398).  Returns the number of output samples written (>= 0, possibly 0) or < 0.
 * out_capacity must be at least lrhip_chain_push_bound(c, n_in).
 * lrhip_chain_flush(): launch the partly filled slot, wait for everything in flight and return the remaining outputs
 * (out_capacity >= lrhip_chain_push_bound(c, 0)); the chain can be pushed to again afterwards.  Call at EOF / cleanup(). */
long lrhip_chain_push(lrhip_chain_t *c, const void *in_host, unsigned long n_in, void *out_host, unsigned long out_capacity);
long lrhip_chain_flush(lrhip_chain_t *c, void *out_host, unsigned long out_capacity);
unsigned long lrhip_chain_push_bound(const lrhip_chain_t *c, unsigned long n_in);
/* Latency bound for LIVE flow graphs (an SDR source at 1.1 MS/s needs ~1 s to fill a 2^20-sample batch; an audio-rate chain minutes):
 * when the oldest sample pushed and not yet launched has waited max_seconds (wall clock, checked at every push), push() launches the
 * partial batch and returns its output from the same call.  0 (the default) = batches run only when full (file / benchmark sources,
 * which deliver faster than real time).  Sample values do not depend on where batches are cut. */
int  lrhip_chain_set_latency(lrhip_chain_t *c, double max_seconds);
/* The wall-clock side of that bound, for a source that STALLS: push() can only look at the clock when it is called, so a live graph whose
 * upstream goes quiet would leave the partial batch unlaunched, where the reference streams every chunk through as it arrives
 * (radio/core/block.lua:575-602).  The host waits for input at most lrhip_chain_poll_due() seconds (-1: nothing pending or no latency bound -
 * wait forever, as PipeMux:_read_single does, radio/core/pipe.lua:495-533; 0: due now) and calls lrhip_chain_poll() when that wait timed
 * out: a partial batch whose oldest sample has waited max_seconds is launched and its output returned from the call, finished batches are
 * handed out either way, and with nothing due it returns 0 at once.  out_capacity >= lrhip_chain_push_bound(c, 0). */
long lrhip_chain_poll(lrhip_chain_t *c, void *out_host, unsigned long out_capacity);
double lrhip_chain_poll_due(const lrhip_chain_t *c);
/* Number of kernels launched by the last chain execute (diagnostic for the fusion tests). */
int lrhip_chain_last_launches(const lrhip_chain_t *c);

/* ---- time-axis sharding: G partitions of ONE stream, each on its own GPU (or as G virtual partitions on one) -------------------------
 * The reference runs a block as one process over the whole stream (radio/core/block.lua:572-590); on a node with 8 GPUs a long
 * recording can be cut into G contiguous partitions instead, because every piece of cross-chunk state of the hot path is either a
 * closed-form function of the ABSOLUTE sample index (rotator phase = omega * n, frequencytranslator.lua:93-110; downsampler phase
 * = n mod D, downsampler.lua:45-56) or a bounded memory of the input (filter history M-1 samples, firfilter.lua:244-250;
 * the discriminator's previous sample, frequencydiscriminator.lua:74; a decaying recurrence's state, iirfilter.lua:113-181).
 *   lrhip_stage_seek / lrhip_chain_seek(c, n0): forget all carried samples and set the absolute counters as if n0 input samples
 *       had been consumed.  The next execute() is then sample n0 of the stream.
 *   lrhip_chain_halo(c): the number of input samples H a partition has to replay in front of its first own sample - seek(n0 - H),
 *       execute(x[n0-H .. n0)) with the output discarded - so that every carried state equals the uninterrupted stream's (filter
 *       histories exactly; recurrences to Float32 underflow of their zero start).  -1 (with lrhip_strerror) when a stage of the
 *       chain has unbounded memory (AGC, frequency modulator, a recurrence that does not decay): such a chain cannot be sharded
 *       in time.  Outputs of the partition [n0, n1) are then the same VALUES as samples of the single-stream run (to the Float32
 *       rounding stated at lrhip_chain_create: <= 1e-7 for the default single-launch receiver and overlap-save filters); with
 *       partition boundaries on multiples of lrhip_chain_shard_align(c) input samples AND a chain built with LRHIP_CHAIN_NO_SINGLE_LAUNCH
 *       (or LRHIP_CHAIN_EXACT) on direct-form filters also bit for bit.
 *   lrhip_chain_shard_align(c): partition boundaries on multiples of this many input samples give every scan kernel of the chain the
 *       tile grid of the uninterrupted run (1 for chains of filters / rotators / discriminators / downsamplers; 5 120 for a tuner
 *       fused with the discriminator behind it, whose tiles are rotated relative to their first sample; 128 000 for the WBFM receiver:
 *       the lcm of that and of the 2 560 audio samples x 25 of its tail). */
int  lrhip_stage_seek(lrhip_stage_t *q, unsigned long long n0);
int  lrhip_chain_seek(lrhip_chain_t *c, unsigned long long n0);
long lrhip_chain_halo(const lrhip_chain_t *c);
unsigned long lrhip_chain_shard_align(const lrhip_chain_t *c);
/* All of the above for a partition that owns the stream from `first_sample` on: seeks to the aligned sample s <= first_sample - halo
 * (returned in *seek_sample: the source has to deliver the stream from s on) and arms the chain to DROP the output of the first
 * (first_sample - s) input samples it is given - by execute, submit or push alike - so the caller's first output sample is the one the
 * single-stream run produces for input sample first_sample.  < 0 for chains with unbounded memory. */
int  lrhip_chain_start_at(lrhip_chain_t *c, unsigned long long first_sample, unsigned long long *seek_sample);

/* ---- fan-out across processes / GPUs below the host language (radio/core/pipe.lua:617-627: one output port, several readers) -------
 * LuaRadio runs every block in its own process; with one process per GPU the source's slab has to reach the other processes' devices
 * without a host round trip.  These are the HIP primitives for that, wrapped so that a LuaJIT host needs no HIP headers:
 *   a consumer process allocates its slab buffers (lrhip_malloc) and exports them (64-byte handles, sent over the control socket the
 *   host already has); the producer opens them and pushes each slab with lrhip_peer_copy on its COPY stream, then records an
 *   interprocess event the consumer waits on (on the GPU, lrhip_ipc_event_wait: no host synchronisation) before its chain reads the
 *   slab.  Two slabs per consumer double-buffer the copy of slab k+1 against the kernels on slab k; a second event per slab, recorded
 *   by the consumer after its chain and waited on by the producer, returns the buffer.  Over xGMI a receiving GPU is bounded by one
 *   link (about 153 GB/s = 19 GS/s of ComplexFloat32). */
enum { LRHIP_IPC_HANDLE_BYTES = 64 };          /* size of the opaque handles below */
int   lrhip_ipc_export(const void *dev_ptr, void *handle_out);                 /* hipIpcGetMemHandle */
void *lrhip_ipc_open(const void *handle);                                       /* hipIpcOpenMemHandle (lazy peer access) */
int   lrhip_ipc_close(void *dev_ptr);
typedef struct lrhip_ipc_event lrhip_ipc_event_t;
lrhip_ipc_event_t *lrhip_ipc_event_create(void *handle_out);                   /* interprocess event + its 64-byte handle */
lrhip_ipc_event_t *lrhip_ipc_event_open(const void *handle);
void  lrhip_ipc_event_destroy(lrhip_ipc_event_t *e);
int   lrhip_ipc_event_record(lrhip_ipc_event_t *e, int on_copy_stream);         /* on the copy stream (1) or the library stream (0) */
int   lrhip_ipc_event_wait(lrhip_ipc_event_t *e, int on_copy_stream);           /* the stream waits on the GPU; the host does not block */
int   lrhip_ipc_event_query(lrhip_ipc_event_t *e);                              /* 1 done, 0 pending, < 0 error */
int   lrhip_ipc_event_synchronize(lrhip_ipc_event_t *e);                        /* host wait */
/* dst/src may live on different devices (peer access is enabled on first use); asynchronous on the library's copy stream */
int   lrhip_peer_copy(void *dst, int dst_device, const void *src, int src_device, unsigned long bytes);
int   lrhip_copy_stream_synchronize(void);

/* ---- device memory helpers for FFI callers that want resident vectors ------------------------------------- */
void *lrhip_malloc(unsigned long bytes);
void  lrhip_free(void *dev_ptr);
int   lrhip_memcpy_h2d(void *dev_dst, const void *host_src, unsigned long bytes);
int   lrhip_memcpy_d2h(void *host_dst, const void *dev_src, unsigned long bytes);
/* device-to-device, asynchronous on the library stream (non-overlapping ranges) */
int   lrhip_memcpy_d2d(void *dev_dst, const void *dev_src, unsigned long bytes);
/* Pinned host vectors (what radio/core/vector.lua's platform.alloc would return for device-fed blocks). */
void *lrhip_host_alloc(unsigned long bytes);
void  lrhip_host_free(void *host_ptr);
/* Zero-copy for vectors the CALLER owns: LuaRadio's owning vectors are page-aligned and long-lived (posix_memalign, radio/core/vector.lua:19-37), its pipe
 * read buffers likewise (platform.alloc, radio/core/pipe.lua:72-76).  A registered range is pinned where it lies (hipHostRegister); the synchronous
 * host-pointer entry points (lrhip_stage_execute, lrhip_chain_execute) then DMA from / to it directly instead of staging through the library's own pinned
 * buffers - whenever the WHOLE input (or output) vector of a call lies inside one registered range.  The owner unregisters before it frees or reallocates
 * (a Vector that grew: radio/core/vector.lua:108-136).  Registrations do not survive fork().  Unregistered vectors work as before.
 * Round 5: with BOTH vectors of a call registered, a stage or chain whose first kernel reads its input once and whose last kernel writes its output once
 * (the FIR forms, Tuner / Decimator, the FM receiver) is handed the host vectors themselves - its loads and stores cross the link, one launch per call, no
 * staging on the device.  The values are those of the same call on device-resident vectors (an overlap-save filter sees the call as ONE chunk, where the
 * staged path cuts calls of 2^20 samples and more into pieces that are chunks of their own: Float32 rounding apart, include the statement above).
 * Round 6: the same for FrequencyTranslator, Downsampler and the complex -> real element-wise blocks (where it measured faster than the staged pipeline);
 * NOT for a filter created with the reference's block-emission framing (use_fft = 1: it copies its input first), and not when the input and output ranges
 * of a call overlap (an in-place call is served by the staged path, as one piece: the whole input is on the device before the first output byte returns). */
int   lrhip_host_register(void *host_ptr, unsigned long bytes);
int   lrhip_host_unregister(void *host_ptr);

/* ---- timing on the library stream (HIP events; used by bench.py for the roofline figure) ------------------- */
typedef struct lrhip_timer lrhip_timer_t;
lrhip_timer_t *lrhip_timer_create(void);
void  lrhip_timer_destroy(lrhip_timer_t *t);
int   lrhip_timer_start(lrhip_timer_t *t);   /* records an event on the current stream */
int   lrhip_timer_stop(lrhip_timer_t *t);    /* records the closing event */
double lrhip_timer_elapsed_ms(lrhip_timer_t *t);   /* waits for the closing event; < 0 on error */

#ifdef __cplusplus
}
#endif
#endif /* LRHIP_H */
