/*
 * algodsp.h — C ABI of the MI355X-native block-DSP engine (libalgodsp_hip.so).
 *
 * This is the drop-in boundary for the sample-buffer hot path of
 * github.com/cwbudde/algo-dsp (pure Go, reference snapshot 2026-03-06).  Every
 * entry point names the reference API it replaces as `file:line` relative to
 * the reference repository root.  A cgo binding for each is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers + int64 sizes only; no C++/torch types cross the boundary;
 *  - every fallible call returns an int status (AD_OK = 0); the sentinel codes
 *    mirror the reference's `errors.Is` targets so the Go side can map them
 *    back (conv.go:41-46, partitioned.go:11-15);
 *  - host-pointer calls copy in and out inside the call (cgo forbids C from
 *    retaining Go pointers); `*_device` calls take device pointers and a HIP
 *    stream (`void*`, NULL = the HIP default stream, as in the HIP API) and are
 *    asynchronous with respect to the host;
 *  - Device buffers.  Every `*_device` call takes rows of `len` elements at a
 *    row stride counted in elements ([channels][stride]; a one-shot call's
 *    array is one row).  For all of them:
 *    1. alignment: any 8-byte-aligned double* (2-byte-aligned uint16_t* for
 *       ad_decode_f16_device) and any stride >= the row length are accepted;
 *       16-byte alignment and even strides are faster, never required;
 *    2. extent: a buffer of C rows is (C-1)*stride + len elements, not
 *       C*stride -- nothing after the last row's len elements is touched;
 *    3. reads: only [c*stride, c*stride + len) of each input row is read, no
 *       other element can influence a result, and an out-of-place call leaves
 *       its input bit-unchanged;
 *    4. writes: only the documented output range of each row is written --
 *       out_len elements, [out_begin, min(out_end, out_len)) for the segment
 *       and mix calls, n elements for the in-place calls; every other byte of
 *       the caller's (the padding between rows, the memory before the base
 *       and after the last row) keeps its bits;
 *    5. layout independence: for a fixed handle configuration and fixed
 *       lengths the results do not depend on base alignment or strides; they
 *       are bit-identical to the contiguous, 16-byte-aligned call.
 *    Input and output may be the same buffer only where a call says so (the
 *    in-place calls; ad_fir_process_device with d_dst == d_src).
 *  - a handle is single-caller, like the reference types (no internal locks);
 *  - ad_last_error() returns a thread-local description of the last failure.
 *  - there is no CPU fallback: with no usable GPU the create calls fail with
 *    AD_ERR_NO_DEVICE.
 */
#ifndef ALGODSP_H_
#define ALGODSP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define AD_OK 0
#define AD_ERR_EMPTY_INPUT 1              /* conv.ErrEmptyInput        conv.go:42 */
#define AD_ERR_EMPTY_KERNEL 2             /* conv.ErrEmptyKernel       conv.go:43 */
#define AD_ERR_LENGTH_MISMATCH 3          /* conv.ErrLengthMismatch    conv.go:44 */
#define AD_ERR_INVALID_BLOCK_SIZE 4       /* conv.ErrInvalidBlockSize  conv.go:45 */
#define AD_ERR_INVALID_BLOCK_ORDER 5      /* conv.ErrInvalidBlockOrder partitioned.go:12 */
#define AD_ERR_EMPTY_IMPULSE_RESPONSE 6   /* conv.ErrEmptyImpulseResponse partitioned.go:13 */
#define AD_ERR_STAGE_INDEX_OUT_OF_RANGE 7 /* conv.ErrStageIndexOutOfRange partitioned.go:14 */
#define AD_ERR_INVALID_ARGUMENT 8         /* non-sentinel fmt.Errorf validation errors,
                                             e.g. streaming_overlap_save.go:50-52 */
#define AD_ERR_DIVISION_BY_ZERO 9         /* conv.ErrDivisionByZero    deconvolve.go:14 */
#define AD_ERR_UNKNOWN_EFFECT 10          /* effectchain.ErrUnknownEffect chain.go:11 (here: a node
                                             type the GPU graph runtime does not run) */
#define AD_ERR_DEVICE 100                 /* HIP runtime failure */
#define AD_ERR_NO_DEVICE 101              /* no usable gfx950 device */
#define AD_ERR_INTERNAL 102

/* conv.Mode (conv.go:57-69) */
#define AD_MODE_FULL 0
#define AD_MODE_SAME 1
#define AD_MODE_VALID 2

const char* ad_last_error(void);
int ad_version(void);
/* Number of visible HIP devices (0 when none). */
int ad_device_count(int* count);

/* ======================================================================== */
/* dsp/conv                                                                 */
/* ======================================================================== */

typedef struct ad_conv ad_conv;

/* ---- conv.StreamingConvolverT (streaming.go:27-49) ----------------------
 * NewStreamingOverlapSave(kernel, blockSize)   streaming_overlap_save.go:88
 * NewStreamingOverlapAdd(kernel, blockSize)    streaming_overlap_add.go:87
 * Both are zero-latency: out = linear convolution of the stream, block by
 * block.  FFTSize() reports the reference's nextPow2(blockSize+K-1).      */
int ad_conv_stream_ols_create(const double* kernel, int64_t kernel_len, int64_t block_size, int device,
                              ad_conv** out);
int ad_conv_stream_ola_create(const double* kernel, int64_t kernel_len, int64_t block_size, int device,
                              ad_conv** out);
/* ProcessBlockTo(output, input)  streaming_overlap_save.go:152-164,
 * streaming_overlap_add.go:154-168.  in_len/out_len must equal BlockSize()
 * (AD_ERR_LENGTH_MISMATCH otherwise).  in and out may alias.              */
int ad_conv_process_block(ad_conv* h, const double* in, int64_t in_len, double* out, int64_t out_len);

/* ---- float32 instantiations (F = float32, C = complex64 in the reference) --
 * NewStreamingOverlapSave32 streaming_overlap_save.go:94,
 * NewStreamingOverlapAdd32  streaming_overlap_add.go:93,
 * NewPartitionedConvolution32 partitioned.go:340 (+ ProcessBlock :348-396).
 * Same validation, getters, Reset and destroy as the float64 handles; the
 * *_block32 calls take float32 blocks and refuse float64 handles.  Samples
 * are widened exactly to float64, convolved by the float64 engine and
 * rounded once to float32 (never less accurate than the reference's
 * complex64 path).                                                       */
int ad_conv_stream_ols32_create(const float* kernel, int64_t kernel_len, int64_t block_size, int device,
                                ad_conv** out);
int ad_conv_stream_ola32_create(const float* kernel, int64_t kernel_len, int64_t block_size, int device,
                                ad_conv** out);
int ad_conv_process_block32(ad_conv* h, const float* in, int64_t in_len, float* out, int64_t out_len);
int ad_conv_partitioned32_create(const float* kernel, int64_t kernel_len, int min_block_order, int max_block_order,
                                 int device, ad_conv** out);
int ad_conv_partitioned_process_block32(ad_conv* h, const float* in, int64_t in_len, float* out, int64_t out_len);

/* ---- batch conv.OverlapSave / conv.OverlapAdd ---------------------------
 * NewOverlapSave(kernel, fftSize)  overlap_save.go:53-107 (fftSize<=0: auto,
 *   non-power-of-two: AD_ERR_INVALID_BLOCK_SIZE, < 2K: silently raised)
 * NewOverlapAdd(kernel, blockSize) overlap_add.go:44-89 (blockSize<=0: auto)
 * Process/ProcessTo: out_len must be in_len + K - 1 (overlap_save.go:126-272,
 *   overlap_add.go:108-182); empty input -> AD_ERR_EMPTY_INPUT.           */
int ad_conv_ols_create(const double* kernel, int64_t kernel_len, int64_t fft_size, int device, ad_conv** out);
int ad_conv_ola_create(const double* kernel, int64_t kernel_len, int64_t block_size, int device, ad_conv** out);
int ad_conv_process(ad_conv* h, const double* in, int64_t in_len, double* out, int64_t out_len);

/* ---- conv.PartitionedConvolutionT (partitioned.go:27-436) ---------------
 * Output is the linear convolution delayed by Latency() = 2^minBlockOrder.
 * ProcessBlock(input, output) accepts any length (in_len must equal out_len).
 * Stage layout (StageCount/StageInfo) follows partitionIR (:269-332).     */
int ad_conv_partitioned_create(const double* kernel, int64_t kernel_len, int min_block_order, int max_block_order,
                               int device, ad_conv** out);
int ad_conv_partitioned_process_block(ad_conv* h, const double* in, int64_t in_len, double* out, int64_t out_len);
int ad_conv_stage_count(const ad_conv* h);
int ad_conv_stage_info(const ad_conv* h, int index, int64_t* part_size, int64_t* block_count);

/* ---- reverb.ConvolutionReverb (dsp/effects/reverb/convolution.go:16-95) --
 * NewConvolutionReverb(kernel, minBlockOrder): partitioned engine with
 * maxBlockOrder 13, wet = dry = 1, Latency() = 2^minBlockOrder.
 * ProcessInPlace: block[i] = dry*block[i] + wet*reverb(block)[i] (:60-85).
 * Reset/Latency/destroy: the common handle API below.                    */
int ad_conv_reverb_create(const double* kernel, int64_t kernel_len, int min_block_order, int device, ad_conv** out);
int ad_conv_reverb_set_wet_dry(ad_conv* h, double wet, double dry);
int ad_conv_reverb_process_inplace(ad_conv* h, double* block, int64_t n);

/* ---- host-buffer I/O of the batch / multi-channel calls ------------------
 * ad_conv_process and ad_conv_ols_process_multi move host buffers over PCIe
 * in overlapped chunks (no reference counterpart: OverlapSave.Process /
 * ProcessTo, overlap_save.go:126-272, on host memory).  Mode AUTO page-locks
 * the caller's buffers for the call (hipHostRegister; nothing is retained
 * after it returns) when the call moves >= 64 MiB and stages smaller calls
 * through pinned double buffers with `workers` copy threads (0: 8); STAGE and
 * REGISTER force one form (REGISTER falls back to staging if the runtime
 * refuses to lock the pages).  Results are identical in every mode.
 * host_io_profile: wall-time split (ms) of the handle's last host call:
 * page-locking, transfers + compute, unlocking (0 for the staged form's
 * first and last).                                                          */
#define AD_HOST_IO_AUTO 0
#define AD_HOST_IO_STAGE 1
#define AD_HOST_IO_REGISTER 2
int ad_conv_set_host_io(ad_conv* h, int mode, int workers);
int ad_conv_host_io_profile(const ad_conv* h, double* register_ms, double* transfer_ms, double* unregister_ms);

/* Low-latency host calls (streaming blocks of hop >= 2048, partitioned calls
 * of <= 256 samples): how many calls took a pre-enqueued launch and how many
 * pre-enqueued launches timed out (the call then ran ordinary launches).  A
 * handle pre-enqueues only for back-to-back callers, while no other handle
 * has a launch waiting and while the library owns at most 3 streams (they
 * would otherwise share the device's 4 hardware queues with the caller's);
 * a waiting launch gives up after 4 call intervals (1..20 ms).  No reference
 * counterpart (diagnostics).                                              */
int ad_conv_lowlat_stats(const ad_conv* h, int64_t* pre_enqueued, int64_t* timed_out);

/* ---- common handle API -------------------------------------------------- */
int ad_conv_reset(ad_conv* h);   /* Reset(): clears history/tail/FDL state */
int64_t ad_conv_block_size(const ad_conv* h);
int64_t ad_conv_kernel_len(const ad_conv* h);
int64_t ad_conv_fft_size(const ad_conv* h);
int64_t ad_conv_step_size(const ad_conv* h); /* OverlapSave.StepSize (overlap_save.go:115) */
int64_t ad_conv_latency(const ad_conv* h);   /* PartitionedConvolution.Latency (partitioned.go:410) */
void ad_conv_destroy(ad_conv* h);

/* ---- one-shot functions ------------------------------------------------- */
/* conv.Direct / DirectTo (conv.go:76-154): bit-exact input-stationary
 * scatter-add order.  dst has n+m-1 elements.                             */
int ad_conv_direct(const double* a, int64_t n, const double* b, int64_t m, double* dst, int device);
/* conv.DirectTo (conv.go:97-154) on device buffers: d_dst has n+m-1
 * elements; enqueued on `stream` (NULL: the default stream), not synced.  */
int ad_conv_direct_device(const double* d_a, int64_t n, const double* d_b, int64_t m, double* d_dst, void* stream);
/* conv.DirectCircular (conv.go:158-189): n == m, dst has n elements.      */
int ad_conv_direct_circular(const double* a, int64_t n, const double* b, int64_t m, double* dst, int device);
/* conv.Convolve / ConvolveMode (conv.go:194-247).  dst_cap is the capacity
 * of dst; *dst_len receives the result length.                            */
int ad_conv_convolve(const double* a, int64_t n, const double* b, int64_t m, int mode, double* dst, int64_t dst_cap,
                     int64_t* dst_len, int device);

/* ---- multi-channel device-resident engine (offline / many-channel path) --
 * Uniformly partitioned overlap-save with a frequency-domain delay line.
 * kernels: n_ir impulse responses of kernel_len taps each, row-major.
 * hop: partition/hop length (power of two, 64..8192); 0 = auto (min(8192, nextpow2(max(K, 256))).
 * channels: number of channels processed per call; ir_index[c] selects the
 *   IR of channel c (NULL: c % n_ir).
 * max_chunk_blocks: blocks per channel per internal chunk (0 = auto).
 * kernel_len == 1 is a gain: every call of the handle (device, segment, mix,
 * host) computes 0 + h[0] x[t] in one kernel, bit-exact with conv.Direct.  */
int ad_conv_multi_create(const double* kernels, int n_ir, int64_t kernel_len, int64_t hop, int channels,
                         const int32_t* ir_index, int64_t max_chunk_blocks, int device, ad_conv** out);
/* Offline schedule of the device calls below (no reference counterpart: how
 * OverlapSave.Process, overlap_save.go:126-254, is laid out on the GPU).
 * SERIAL: each internal chunk's forward transforms, delay-line MAC and inverse
 * transforms run in turn on the caller's stream.  PIPELINED (hop >= 2048;
 * smaller hops stay serial): chunks of chunk_blocks blocks per channel (0:
 * auto) whose spectra stay in the Infinity Cache, the MAC and the inverse
 * transforms on two internal streams, so consecutive chunks' kernels overlap;
 * the caller's stream still passes the call only when every output is
 * written.  run_blocks: the MAC's run length (0: auto).  Results are
 * bit-identical in both schedules.  Applies from the next signal start (a
 * process_device call, or a segment / mix call with out_begin == 0).       */
#define AD_CONV_SCHED_SERIAL 0
#define AD_CONV_SCHED_PIPELINED 1
#define AD_CONV_SCHED_CHUNKED 2 /* PIPELINED's chunks and rings, every kernel on the caller's stream */
int ad_conv_multi_set_schedule(ad_conv* h, int mode, int64_t chunk_blocks, int64_t run_blocks);
int ad_conv_multi_get_schedule(const ad_conv* h, int* mode, int64_t* chunk_blocks);
/* Long-block plan of ad_conv_multi_process_device: under the SERIAL schedule a
 * whole-signal call with kernel_len <= 2^19 may run as overlap-save over
 * blocks of one 2^21-point real FFT (hop 2^21 - kernel_len + 1) instead of
 * the partitioned engine, which moves about two thirds of the bytes.  AUTO
 * (the default) takes it when out_len spans at least 4 such hops, ON for any
 * such call, OFF never.  The entry points are bit-identical to each other
 * within a plan; a call that takes the long plan differs from the segment,
 * mix and host forms of the same signal in the last bits (both are within the
 * 1e-9 bound), and OFF restores the equality.  The first long call of a handle
 * builds the IR's long spectra and allocates the intermediates (16.9 MB per
 * IR plus 16.9 MB per channel and block), freed with the handle.
 * get_schedule and ad_conv_fft_size do not change.                          */
#define AD_CONV_LONG_AUTO 0
#define AD_CONV_LONG_OFF 1
#define AD_CONV_LONG_ON 2
int ad_conv_multi_set_long_blocks(ad_conv* h, int mode);
int ad_conv_multi_get_long_blocks(const ad_conv* h, int* mode);
/* Full linear convolution of every channel (ModeFull semantics per channel):
 * d_in  [channels][in_stride] (first in_len used),
 * d_out [channels][out_stride] (first out_len written; out_len <= in_len+K-1).
 * Device pointers; asynchronous on `stream` (NULL = default stream).
 * This call and the segment and mix forms below check the rows before any
 * device work: a null d_in / d_out / d_mix -> AD_ERR_INVALID_ARGUMENT; with
 * more than one channel, in_stride < in_len or out_stride < out_len (the mix
 * form: mix_stride < out_len, for any channel count) -> AD_ERR_LENGTH_MISMATCH. */
int ad_conv_multi_process_device(ad_conv* h, const double* d_in, int64_t in_stride, int64_t in_len, double* d_out,
                                 int64_t out_stride, int64_t out_len, void* stream);
/* The same full linear convolution computed one output segment at a time:
 * this call writes d_out[c][out_begin .. min(out_end, out_len)) only.
 * out_begin == 0 starts a new signal; a later segment must start where the
 * previous one ended (the frequency-domain delay line carries over), and
 * out_begin / out_end are multiples of the hop (out_end may also be out_len).
 * Segments let a caller overlap per-segment work, such as the multi-GPU
 * mixdown reduce, with the next segment's convolution.  Results are identical
 * to one ad_conv_multi_process_device call.  No reference counterpart: it is
 * the batch OverlapSave.Process (overlap_save.go:126-254) split by output
 * range.  Out-of-order segments return AD_ERR_INVALID_ARGUMENT.            */
int ad_conv_multi_process_device_segment(ad_conv* h, const double* d_in, int64_t in_stride, int64_t in_len,
                                         double* d_out, int64_t out_stride, int64_t out_len, int64_t out_begin,
                                         int64_t out_end, void* stream);
/* The full linear convolution of every channel with the stereo mixdown of
 * the group fused into the inverse transform (config 4's per-GPU work, SURVEY
 * 8(e)): d_mix [2][mix_stride] receives, for out_begin <= t < out_end,
 *   d_mix[t]              (L) = sum of the channels with an even global index,
 *   d_mix[mix_stride + t] (R) = sum of those with an odd global index,
 * where local channel c has global index first_parity + c (mod 2), summed in
 * increasing c.  The per-channel outputs are not written to memory (hop >=
 * 2048; smaller hops convolve into an internal buffer and mix it).  Equal to
 * ad_conv_multi_process_device + ad_conv_mixdown_device to rounding (each
 * channel's block enters the sum as (acc + A) - W B of its split inverse
 * transform's halves, computed at another radix split).  out_begin /
 * out_end follow ad_conv_multi_process_device_segment (out_end <= 0: out_len;
 * 0, 0 = the whole output in one call).  A caller mixing into the RCCL reduce
 * then passes channels = 0 to ad_mixdown_reduce.  Reference: the batch
 * OverlapSave.Process (overlap_save.go:126-254) per channel, then the mix.  */
int ad_conv_multi_process_device_mix(ad_conv* h, const double* d_in, int64_t in_stride, int64_t in_len,
                                     double* d_mix, int64_t mix_stride, int64_t out_len, int first_parity,
                                     int64_t out_begin, int64_t out_end, void* stream);
/* OverlapSave.Process / ProcessTo (overlap_save.go:126-272) of every channel
 * of a multi-channel handle on HOST buffers: in[c] holds n samples, out[c]
 * receives n + kernel_len - 1.  The signal crosses PCIe in chunks through
 * pinned double buffers, overlapping H2D of chunk i+1, the convolution of
 * chunk i and D2H of chunk i-1 (three streams); bit-identical to the device
 * call.  channels must equal the handle's (else AD_ERR_LENGTH_MISMATCH).    */
int ad_conv_ols_process_multi(ad_conv* h, const double* const* in, double* const* out, int channels, int64_t n);

/* ---- multi-channel streaming convolver ----------------------------------
 * `channels` StreamingOverlapSave instances (streaming_overlap_save.go:45-184)
 * sharing n_ir kernels (ir_index[c], NULL: c % n_ir) in one handle: each
 * block call runs every channel with ONE launch per engine kernel, the
 * frequency-domain delay line and input history stay on the device between
 * calls (config 4 real-time form: 64 reverb channels, block by block).
 * Any block_size > 0: with a power-of-two divisor >= 256 (or a power of two
 * >= 64) that divisor is the hop and a call is whole engine blocks; any other
 * size (480, 960, 1000, 4800 ...) runs at hop = nextPow2(block_size) (at least
 * kernel_len/64, within 64..8192) and carries the unfinished block between
 * calls, so a call costs at most ceil((hop - 1 + block_size) / hop) FFT
 * blocks per channel.  Zero latency: out = the newest block_size samples of
 * each channel's linear convolution.
 * Reset / getters: ad_conv_reset, ad_conv_block_size, ad_conv_fft_size.   */
int ad_conv_multi_stream_create(const double* kernels, int n_ir, int64_t kernel_len, int64_t block_size,
                                int channels, const int32_t* ir_index, int device, ad_conv** out);
/* host buffers: in[c], out[c] of n == block_size samples (else AD_ERR_LENGTH_MISMATCH) */
int ad_conv_multi_stream_process_block(ad_conv* h, const double* const* in, double* const* out, int channels,
                                       int64_t n);
/* device buffers [channels][stride]; asynchronous on `stream` */
int ad_conv_multi_stream_process_block_device(ad_conv* h, const double* d_in, int64_t in_stride, double* d_out,
                                              int64_t out_stride, void* stream);
/* ---- many-channel partitioned convolution / convolution reverb ----------
 * `channels` PartitionedConvolution instances (partitioned.go:212-436) that
 * share ONE impulse response, device resident: y[c][t] = (h * x_c)[t - 2^minOrder]
 * for any call length.  Each non-uniform stage is one UPOLS engine over all
 * channels (one launch per engine kernel per stage per call), accumulating
 * into a device buffer; latency 2^minOrder must be 64..8192 here.
 * The reverb form (maxBlockOrder 13, wet = dry = 1 until
 * ad_conv_reverb_set_wet_dry) processes in place as
 * ConvolutionReverb.ProcessInPlace (convolution.go:60-85) -- the
 * effect-chain reverb-conv node.  ad_conv_reset, ad_conv_latency,
 * ad_conv_stage_count / ad_conv_stage_info apply.                          */
int ad_conv_pc_multi_create(const double* kernel, int64_t kernel_len, int min_order, int max_order, int channels,
                            int device, ad_conv** out);
int ad_conv_pc_multi_process_device(ad_conv* h, const double* d_in, int64_t in_stride, double* d_out,
                                    int64_t out_stride, int64_t n, void* stream);
int ad_conv_reverb_multi_create(const double* kernel, int64_t kernel_len, int min_order, int channels, int device,
                                ad_conv** out);
int ad_conv_reverb_multi_process_device(ad_conv* h, double* d_buf, int64_t stride, int64_t n, void* stream);
/* host buffer [channels][n], in place */
int ad_conv_reverb_multi_process(ad_conv* h, double* buf, int64_t n);

/* Live kernel timing (HIP events recorded around every launch on the launch
 * stream) for the FFT engine of a handle.  Kernel index: 0 window rFFT,
 * 1 frequency-domain delay-line MAC, 2 inverse rFFT + overlap-save store.
 * read() synchronises and returns, per kernel, the summed duration (ms),
 * the launch count and the algorithmic bytes those launches moved
 * (DESIGN.md), then clears the counters.  Arrays have 3 entries.          */
int ad_conv_profile_enable(ad_conv* h, int enable);
int ad_conv_profile_read(ad_conv* h, double* total_ms, int64_t* launches, double* alg_bytes);
/* Which kernels enabled timing records: bit k = kernel k (default 7, all).
 * Timing one kernel keeps two events per call inside a timed loop.       */
int ad_conv_profile_kernels(ad_conv* h, int mask);
/* Stereo mixdown of a channel group (build-defined; the
 * reference defines no mixdown):
 *   d_mix[t]              (L) = sum of the group's channels with an even global index,
 *   d_mix[mix_stride + t] (R) = sum of those with an odd global index,
 * t < len; channel c of the group has global index first + c and
 * first_parity = first & 1.  d_chan [channels][stride].  Asynchronous on
 * `stream`.  mix_stride >= len (L and R rows of one [2][mix_stride] buffer,
 * so an output segment can be mixed into its place: pass d_chan + b and
 * d_mix + b).                                                              */
int ad_conv_mixdown_device(const double* d_chan, int channels, int64_t stride, int64_t len, double* d_mix,
                           int64_t mix_stride, int first_parity, void* stream);

/* ---- multi-GPU mixdown over RCCL (SURVEY 8(b) ad_mixdown_reduce, 8(e)) ----
 * One process per GPU; every rank convolves its own channel group and the
 * stereo partial mixes are summed on `root` with ONE RCCL reduce over xGMI.
 * The communicator is created from a unique id that rank 0 makes and the
 * caller distributes (cgo side: any transport -- the reference has no
 * multi-process layer).  librccl.so.1 is loaded on first use (no link-time
 * dependency for single-GPU callers).                                      */
#define AD_COMM_ID_BYTES 128
typedef struct ad_comm ad_comm;
int ad_comm_get_unique_id(uint8_t id[AD_COMM_ID_BYTES]);
/* ncclCommInitRank over `nranks` ranks; `device` is this rank's GPU. */
int ad_comm_create(const uint8_t id[AD_COMM_ID_BYTES], int nranks, int rank, int device, ad_comm** out);
void ad_comm_destroy(ad_comm* comm);
int ad_comm_rank(const ad_comm* comm);
int ad_comm_size(const ad_comm* comm);
/* k_mixdown of this rank's group into d_mix ([2][mix_stride], as
 * ad_conv_mixdown_device), then an in-place sum-reduce of d_mix's 2 x len
 * values to `root` (d_mix on root holds the whole job's stereo mix; on the
 * other ranks it holds the rank's partial mix).  Both are enqueued on
 * `stream` and the call returns without waiting.  channels == 0 skips the
 * mixdown (d_mix already holds the partial mix, e.g. a stereo group).      */
int ad_mixdown_reduce(ad_comm* comm, const double* d_chan, int channels, int64_t stride, int64_t len,
                      int first_parity, double* d_mix, int64_t mix_stride, int root, void* stream);

/* ======================================================================== */
/* dsp/filter, dsp/effects: per-sample processors                           */
/* ======================================================================== */

/* ---- effect chain: biquad EQ -> Compressor -> Freeverb, per channel ------
 * One handle runs `channels` independent instances of the reference
 * processors, each stage optional, fused per sample on the GPU (bit-exact
 * with running the stages block by block, as effectchain.Chain.Process does,
 * chain_process.go:11-33).  Buffers are [channels][n] (host) or
 * [channels][stride] (device), processed in place.
 *
 * EQ stage = biquad.Chain(s) (chain.go:6-138, section.go:26-155): a table of
 * sections {pre_gain, b0, b1, b2, a1, a2}; pre_gain is the Chain gain on a
 * chain's first section (1.0 otherwise).  per_channel = 0: one table [nsec][6]
 * for all channels; 1: [channels][nsec][6].  Replaces Chain.ProcessBlock and,
 * with one section, Section.ProcessBlock (the avx2/generic registry kernels,
 * registry.go:10-100, compute the same DF-II-T recurrence).
 * Compressor stage = dynamics.Compressor ProcessInPlace (compressor.go:362-366)
 * configured by an ad_compressor_config struct, mirroring the setters
 * (compressor.go:130-305).
 * Freeverb stage = reverb.Reverb ProcessInPlace (reverb.go:185-189) with
 * SetWet/SetDry/SetRoomSize/SetDamp/SetGain values (reverb.go:192-220).     */
typedef struct ad_fx_chain ad_fx_chain;
typedef struct ad_compressor_config {
  double sample_rate, threshold_db, ratio, knee_db, attack_ms, release_ms, rms_window_ms, makeup_db;
  double sidechain_low_cut_hz, sidechain_high_cut_hz; /* 0: off; else [1 Hz, Nyquist), low < high */
  int topology;             /* 0 feed-forward, 1 feedback */
  int detector_mode;        /* 0 peak, 1 RMS */
  int feedback_ratio_scale; /* 1: feedback topology scales time constants and ratio */
  int auto_makeup;          /* 1: makeup = -threshold*(1-1/ratio) */
} ad_compressor_config;
/* Non-finite detector levels (an Inf or NaN sample, or a square that overflows
 * in the RMS detector).  The envelope follower computes the reference's map
 * env + k (src - env), k = attack or 1 - release, as two FMAs with
 * c2 = (attack - (1 - release)) / 2 (csrc/dsp_device.hpp env_step).  With
 * c2 > 0 (the attack coefficient above 1 - release coefficient: any attack
 * faster than the release) it gives the reference's result on a non-finite
 * level too: the same NaN samples and the same exact zeros afterwards.  With
 * c2 <= 0 (an attack as slow as the release, or slower) an infinite level
 * makes the envelope Inf - Inf = NaN, and the output is NaN from that sample
 * until Reset(), where the reference's envelope stays +Inf and its output is
 * exact zeros.  The deviation is kept: the select that would remove it sits on
 * the two-FMA envelope chain, the chain's longest recurrence.
 * Channels are independent: a poisoned channel never changes another one. */
/* NewCompressor(sampleRate) defaults (compressor.go:77-127). */
void ad_compressor_default_config(ad_compressor_config* cfg, double sample_rate);
/* The setters' validation of a whole config, host only (no device needed):
 * AD_OK, or AD_ERR_INVALID_ARGUMENT for any value a reference setter rejects:
 * ratio outside [1, 100], knee outside [0, 24] dB, attack outside [0.1, 1000]
 * ms, release outside [1, 5000] ms, RMS window outside [1, 1000] ms
 * (compressor.go:16-23, core.go:10-12, 131-198), a non-finite threshold or
 * makeup, a bad sample rate, topology or detector mode, a side-chain cut
 * that is negative or not in [1 Hz, Nyquist), or low >= high when both are on
 * (core.go:542-564).  ad_fx_chain_set_compressor and the graph's COMPRESSOR
 * node run the same check and change nothing on failure. */
int ad_compressor_validate(const ad_compressor_config* cfg);

int ad_fx_chain_create(int channels, int device, ad_fx_chain** out);
int ad_fx_chain_set_eq(ad_fx_chain* h, const double* sections, int nsec, int per_channel);
/* The EQ round-off noise estimate ad_fx_chain_set_eq computes for the engine
 * choice (eps sqrt(sum NG) of the worst of `sets` tables [nsec][6]; +inf when
 * a section is unstable: |a2| >= 1 or |a1| >= 1 + a2).  Host only, no device
 * needed; no reference counterpart (diagnostics).                         */
int ad_fx_eq_noise(const double* sections, int nsec, int sets, double* noise);
/* The first configuration of the dynamics stage starts it from Reset().  A
 * later call is the reference's setters (core.go:101-250): the envelope, the
 * feedback memory, the metrics and the gate's hold counter carry on; a changed
 * RMS window length (in samples) restarts the RMS ring, index, fill and sum
 * only, in either detector mode (core.go:500-518); a side-chain cut set to 0
 * zeroes that filter's state (core.go:606-650). */
int ad_fx_chain_set_compressor(ad_fx_chain* h, const ad_compressor_config* cfg); /* NULL: stage off */
/* dynamics.Expander / dynamics.Gate (expander.go, gate.go) as the chain's
 * dynamics stage instead of the compressor: cfg gives threshold, ratio, knee,
 * attack, release, detector, topology, RMS window and side-chain filters
 * (makeup fields ignored: these have none); range_db is SetRange, hold_ms is
 * the gate's SetHold (gate != 0).  Out-of-range values -> AD_ERR_INVALID_ARGUMENT
 * (the setters' validation). */
int ad_fx_chain_set_expander(ad_fx_chain* h, const ad_compressor_config* cfg, int gate, double range_db,
                             double hold_ms);
int ad_fx_chain_set_freeverb(ad_fx_chain* h, double wet, double dry, double room_size, double damp, double gain);
int ad_fx_chain_disable_freeverb(ad_fx_chain* h);
int ad_fx_chain_reset(ad_fx_chain* h); /* Chain/Compressor/Reverb Reset() */
int ad_fx_chain_process(ad_fx_chain* h, double* buf, int64_t n);
int ad_fx_chain_process_device(ad_fx_chain* h, double* d_buf, int64_t stride, int64_t n, void* stream);
/* Compressor metrics of one channel (updateMetrics compressor.go:411-423):
 * input peak, output peak, minimum gain (gain reduction, linear). */
int ad_fx_chain_compressor_metrics(ad_fx_chain* h, int channel, double* input_peak, double* output_peak,
                                   double* gain_reduction);
/* Compressor.ResetMetrics (compressor.go:389-391) of every channel: the peaks
 * to 0, the gain reduction to 1; the dynamics state is not touched. */
int ad_fx_chain_reset_compressor_metrics(ad_fx_chain* h);
/* EQ section state [channels][nsec][2] {d0, d1} (Chain.State, chain.go:122-130). */
int ad_fx_chain_eq_state(ad_fx_chain* h, double* state, int64_t cap);
/* Chain.SetState (chain.go:130-138) / Section.SetState (section.go:152-155)
 * of every channel, between calls: state [channels][nsec][2] {d0, d1};
 * n < channels*nsec*2 -> AD_ERR_LENGTH_MISMATCH (the reference indexes
 * states[i] for every section).  With ad_fx_chain_eq_state this is the
 * reference's checkpoint / resume surface for the EQ.                       */
int ad_fx_chain_set_eq_state(ad_fx_chain* h, const double* state, int64_t n);
/* Which engine runs the chain:
 *   AUTO            with a compressor, the time-parallel engine (below);
 *                   otherwise the staged engine (stage kernels over time
 *                   chunks on three streams, fx_staged.hip) where it applies
 *                   -- feed-forward dynamics, <= 8 EQ sections, <= 8192
 *                   channels with Freeverb -- with the EQ split over two CUs
 *                   when >= 3 sections are on; else FUSED;
 *   FUSED           the fused per-sample kernels (dsp_kernels.hip k_chain*);
 *   STAGED_NOSPLIT  staged, one EQ pipeline per channel group;
 *   STAGED          staged with the split EQ stage;
 *   TIME_PARALLEL   the time-parallel engine (fx_tp.hip) also for chains
 *                   without a compressor: EQ only, Freeverb only, EQ +
 *                   Freeverb (where the staged engine applies; otherwise as
 *                   AUTO).
 * FUSED, STAGED_NOSPLIT and STAGED perform the reference's operations in its
 * order: their outputs are identical.  The time-parallel engine starts the
 * EQ's time segments from chained states (double-double): its outputs are
 * within 1e-12 relative RMS of those (the serial recurrence's own rounding
 * noise for low-frequency sections), not bit-identical.  That noise grows
 * with the sections' round-off noise gain (poles near z = 1: a low highpass
 * at a high sample rate), so AUTO and TIME_PARALLEL keep the staged engine
 * for an EQ whose noise estimate exceeds 4.5e-13 (ad_fx_chain_last_engine).
 * chunk: samples per staged / time-parallel chunk (0: the engine's default;
 * otherwise >= 256).                                                         */
#define AD_FX_ENGINE_AUTO 0
#define AD_FX_ENGINE_FUSED 1
#define AD_FX_ENGINE_STAGED_NOSPLIT 2
#define AD_FX_ENGINE_STAGED 3
#define AD_FX_ENGINE_TIME_PARALLEL 4
int ad_fx_chain_set_engine(ad_fx_chain* h, int engine, int64_t chunk);
/* The engine that ran the last process call (AD_FX_ENGINE_FUSED, _STAGED,
 * _STAGED_NOSPLIT or _TIME_PARALLEL; -1 before the first call) and the EQ's
 * round-off noise estimate eps sqrt(sum NG) that gates the time-parallel
 * engine (0 without an EQ, inf for an unstable section).  Either pointer may
 * be NULL.  No reference counterpart (engine introspection). */
int ad_fx_chain_last_engine(ad_fx_chain* h, int* engine, double* eq_noise);
/* Per-wave clock counters (s_memtime ticks) of the first chunk of each call,
 * for profiling the serial stages: {compute, barrier wait} pairs per wave. */
int ad_fx_chain_set_profiling(ad_fx_chain* h, int enable);
int ad_fx_chain_read_profile(ad_fx_chain* h, unsigned long long* counters, int cap, int* count);
void ad_fx_chain_destroy(ad_fx_chain* h);

/* ---- batched effectchain graph (dsp/effectchain, 8(f)4) -------------------
 * `channels` copies of one effect-chain graph, each with its own state, run
 * together (one lane per channel).  Replaces effectchain.Chain.Process
 * (chain_process.go:11-33) for graphs made of the node types below; the
 * host-side graph compiler (JSON parse + Kahn order, graph.go:57-165, node
 * Configure param clamps, runtime_*.go) lives in the caller and passes the
 * nodes in topological order, node 0 being `_input`.
 * Per node (processNode, chain_process.go:136-175): the input is the
 * average of the parents' outputs (mixParentEdgesInto :295-318: zeros with
 * no parent, a copy for one, sum in edge order * 1/k for k), then
 *   AD_FXN_SPLIT_FREQ  LR crossover: low = LP chain, high = HP chain, read by
 *                      consumers through parent port 0 / 1 (crossover.go:80-94,
 *                      chain_process.go:177-227; not affected by `bypassed`);
 *   AD_FXN_OUTPUT / AD_FXN_PASS ("split", "sum") / bypassed: mix only;
 *   AD_FXN_BIQUAD      biquad.Chain.ProcessBlock, sections [nsec][6] as in
 *                      ad_fx_chain_set_eq (filter* nodes, runtime_filter_pitch_reverb.go:186-195);
 *   AD_FXN_COMPRESSOR  Compressor.ProcessInPlace with *comp (dyn-compressor,
 *                      and dyn-limiter = NewLimiter's ratio 100 / attack 0.1 ms /
 *                      hard knee / no makeup config, limiter.go:11-44);
 *   AD_FXN_FREEVERB    reverb.Reverb.ProcessInPlace, verb = {wet, dry,
 *                      room_size, damp, gain} (runtime_filter_pitch_reverb.go:330-345);
 *   AD_FXN_CONV_REVERB reverb.ConvolutionReverb.ProcessInPlace (reverb-conv,
 *                      runtime_misc.go:61-67) on the many-channel partitioned engine;
 *   AD_FXN_FDN_REVERB  reverb.FDNReverb.ProcessInPlace (reverb-fdn,
 *                      runtime_filter_pitch_reverb.go:366-368) on the FDN kernel;
 *   AD_FXN_DELAY       effects.Delay.ProcessInPlace (delay), or with *delay in
 *                      mode 1 the integer delay of delay-simple
 *                      (runtime_modulation.go:304-362);
 *   AD_FXN_FLANGER     modulation.Flanger.ProcessInPlace (flanger,
 *                      runtime_modulation.go:34-52);
 *   AD_FXN_PHASER / AD_FXN_TREMOLO / AD_FXN_RINGMOD  the ProcessInPlace of
 *                      modulation.Phaser, Tremolo and RingModulator (phaser,
 *                      tremolo, ringmod, runtime_modulation.go:54-69, 259-302),
 *                      configured through ad_fx_graph_create_ext;
 *   AD_FXN_DISTORTION  effects.Distortion.ProcessInPlace (distortion and
 *                      dist-cheb, runtime_modulation.go:91-171) and
 *   AD_FXN_BITCRUSHER  effects.BitCrusher.ProcessInPlace (bitcrusher,
 *                      runtime_modulation.go:71-89),
 *   AD_FXN_DEESSER     dynamics.DeEsser.ProcessInPlace (dyn-deesser,
 *                      runtime_dynamics.go:240-314) and
 *   AD_FXN_TRANSIENT   dynamics.TransientShaper.ProcessInPlace (dyn-transient,
 *                      runtime_dynamics.go:316-351),
 *   AD_FXN_SPECFREEZE  effects.SpectralFreeze.ProcessInPlace (spectral-freeze,
 *                      runtime_filter_pitch_reverb.go:274-303) and
 *   AD_FXN_PITCHSPEC   pitch.SpectralPitchShifter.ProcessInPlace (pitch-spectral,
 *                      runtime_filter_pitch_reverb.go:248-272), configured through
 *                      ad_fx_graph_create_cfg, and
 *   AD_FXN_PITCHTIME   pitch.PitchShifter.ProcessInPlace (pitch-time,
 *                      runtime_filter_pitch_reverb.go:222-246), configured the same way.
 * The result is the output node's buffer.  Linear runs of in-place nodes fuse
 * into one launch (bit-identical, see capi_fxgraph.cpp).  Other node types
 * return AD_ERR_UNKNOWN_EFFECT; the configs are copied at create.          */
#define AD_FXN_INPUT 0
#define AD_FXN_OUTPUT 1
#define AD_FXN_PASS 2
#define AD_FXN_SPLIT_FREQ 3
#define AD_FXN_BIQUAD 4
#define AD_FXN_COMPRESSOR 5
#define AD_FXN_FREEVERB 6
#define AD_FXN_CONV_REVERB 7 /* reverb-conv (runtime_misc.go:12-67): ConvolutionReverb(ir, conv_min_order)
                                with SetWetDry(conv_wet, conv_dry), in place; the caller
                                mono-averages the provider's IR as Configure does */
#define AD_FXN_FDN_REVERB 8 /* reverb-fdn, and reverb with model "fdn" (runtime_filter_pitch_reverb.go:347-395):
                               FDNReverb.ProcessInPlace configured by *fdn (ad_fdn_config, below), an op
                               of its own on the many-channel FDN kernel */
#define AD_FXN_DELAY 9   /* delay and delay-simple: an ad_delay created from *delay (below), an op of its own */
#define AD_FXN_FLANGER 10 /* flanger: an ad_flanger created from *flanger (below), an op of its own */
#define AD_FXN_PHASER 11  /* phaser: an ad_phaser created from ext[i].phaser, an op of its own */
#define AD_FXN_TREMOLO 12 /* tremolo: an ad_tremolo created from ext[i].tremolo, an op of its own */
#define AD_FXN_RINGMOD 13 /* ringmod: an ad_ringmod created from ext[i].ringmod, an op of its own */
/* 14 is not assigned: it stays AD_ERR_UNKNOWN_EFFECT */
#define AD_FXN_DISTORTION 15 /* distortion and dist-cheb: an ad_distortion created from cfg[i], an op of its own */
#define AD_FXN_BITCRUSHER 16 /* bitcrusher: an ad_bitcrusher created from cfg[i], an op of its own */
/* 17 is not assigned: it stays AD_ERR_UNKNOWN_EFFECT */
#define AD_FXN_DEESSER 18   /* dyn-deesser: an ad_deesser created from cfg[i], an op of its own */
#define AD_FXN_TRANSIENT 19 /* dyn-transient: an ad_transient created from cfg[i], an op of its own */
#define AD_FXN_SPECFREEZE 20 /* spectral-freeze: an ad_specfreeze created from cfg[i] (its window table is read
                                at create), an op of its own */
#define AD_FXN_PITCHSPEC 21  /* pitch-spectral: an ad_pitchspec created from cfg[i] (its window and resampling
                                prototype are read at create), an op of its own */
/* 22 is not assigned: it stays AD_ERR_UNKNOWN_EFFECT */
#define AD_FXN_LOOKAHEAD 23  /* dyn-lookahead: an ad_lookahead created from cfg[i] (an ad_fx_lookahead_node), an op
                                of its own that reads its side parents */
#define AD_FXN_VOCODER 24    /* vocoder: an ad_vocoder created from cfg[i] (an ad_fx_vocoder_node); the node's
                                buffer is the modulator, the side parents mix into the carrier */
#define AD_FXN_PITCHTIME 25  /* pitch-time: pitch.PitchShifter.ProcessInPlace (runtime_filter_pitch_reverb.go:222-246)
                                configured by cfg[i], an ad_pitchtime_config, see below (its fade-in table is read
                                at create), an op of its own.  The node has no handle type and no entry points of its
                                own: a graph of input -> pitch-time -> output is the processor */
#define AD_FX_MAX_PARENTS 8
struct ad_fdn_config;
struct ad_delay_config;
struct ad_flanger_config;
typedef struct ad_fx_node {
  int type;
  int bypassed;
  int n_parents;
  const int32_t* parents;      /* indices of earlier nodes, in the graph's edge order */
  const int32_t* parent_ports; /* NULL: all 0; 1 = a split-freq node's high band */
  const double* sections;      /* BIQUAD: [nsec][6]; SPLIT_FREQ: low-band (LP) chain */
  int nsec;
  const double* sections2;     /* SPLIT_FREQ: high-band (HP) chain [nsec2][6] */
  int nsec2;
  const ad_compressor_config* comp; /* COMPRESSOR */
  double verb[5];                   /* FREEVERB: wet, dry, room_size, damp, gain */
  int dyn_mode;                     /* COMPRESSOR: 0 compressor / limiter, 1 expander (dyn-expander),
                                       2 gate (dyn-gate); see ad_fx_chain_set_expander */
  double dyn_range_db, dyn_hold_ms; /* expander / gate: SetRange, the gate's SetHold */
  const double* ir;                 /* CONV_REVERB: impulse response [ir_len] */
  int64_t ir_len;
  int conv_min_order;               /* CONV_REVERB: minBlockOrder (reverb-conv uses 7; maxBlockOrder 13) */
  double conv_wet, conv_dry;        /* CONV_REVERB: SetWetDry(wet, dry) (reverb-conv: wet param, dry 1.0) */
  const struct ad_fdn_config* fdn;  /* FDN_REVERB */
  const struct ad_delay_config* delay;     /* DELAY */
  const struct ad_flanger_config* flanger; /* FLANGER */
} ad_fx_node;
/* Configurations of the node types added after ad_fx_node was laid out; ext[i] belongs to nodes[i]. */
struct ad_phaser_config;
struct ad_tremolo_config;
struct ad_ringmod_config;
typedef struct ad_fx_node_ext {
  const struct ad_phaser_config* phaser;   /* PHASER */
  const struct ad_tremolo_config* tremolo; /* TREMOLO */
  const struct ad_ringmod_config* ringmod; /* RINGMOD */
} ad_fx_node_ext;
typedef struct ad_fx_graph ad_fx_graph;
int ad_fx_graph_create(const ad_fx_node* nodes, int n_nodes, int channels, int device, ad_fx_graph** out);
/* The same with ext [n_nodes] (NULL: none, which is ad_fx_graph_create).  A PHASER, TREMOLO or RINGMOD
 * node without its configuration is AD_ERR_INVALID_ARGUMENT, through either entry point. */
int ad_fx_graph_create_ext(const ad_fx_node* nodes, const ad_fx_node_ext* ext, int n_nodes, int channels, int device,
                           ad_fx_graph** out);
/* The configuration transport of the node types after RINGMOD: cfg[i] belongs to nodes[i] and holds the
 * node type's own config structure (DISTORTION: ad_distortion_config, BITCRUSHER: ad_bitcrusher_config,
 * DEESSER: ad_deesser_config, TRANSIENT: ad_transient_config) with its size, so a later node type needs
 * neither a new structure nor a new entry point.  cfg NULL: none, which is ad_fx_graph_create_ext.  A
 * DISTORTION, BITCRUSHER, DEESSER or TRANSIENT node without its configuration, with bytes other than the
 * size of its structure, or with a configuration its validate refuses is AD_ERR_INVALID_ARGUMENT, through
 * all three entry points.  The configurations are copied at create. */
typedef struct ad_fx_node_cfg {
  const void* config;
  int64_t bytes;
} ad_fx_node_cfg;
int ad_fx_graph_create_cfg(const ad_fx_node* nodes, const ad_fx_node_ext* ext, const ad_fx_node_cfg* cfg, int n_nodes,
                           int channels, int device, ad_fx_graph** out);
/* buf [channels][n] (host) / [channels][stride] (device), processed in place. */
int ad_fx_graph_process(ad_fx_graph* g, double* buf, int64_t n);
int ad_fx_graph_process_device(ad_fx_graph* g, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_fx_graph_reset(ad_fx_graph* g); /* every node runtime's Reset() */
/* Compiled size: device ops per call, buffers (including the caller's) and
 * streams the independent branches are spread over (the caller's included). */
int ad_fx_graph_op_count(const ad_fx_graph* g, int* launches, int* buffers, int* lanes);
void ad_fx_graph_destroy(ad_fx_graph* g);

/* One-shot biquad.Chain.ProcessBlock over `channels` chains sharing one
 * coefficient set coeffs [sections][5] {b0,b1,b2,a1,a2} and gain (chain.go:59-70);
 * state [channels][sections][2] is read and updated; buf [channels][n]. */
int ad_biquad_chain_process(const double* coeffs, double* state, double gain, double* buf, int channels,
                            int sections, int64_t n, int device);

/* ---- IRLB f16 sample decode (internal/webdemo/irlib.go:68-97, 414-451) ----
 * AUDI chunk payload (little-endian f16, frames interleaved by channel) ->
 * float64 [channels][frames], bit-exact with decodeF16 including its
 * subnormal exponent (every subnormal half decodes to twice its IEEE value). */
int ad_decode_f16(const uint16_t* in, int64_t frames, int channels, double* out, int device);
int ad_decode_f16_device(const uint16_t* d_in, int64_t frames, int channels, double* d_out, void* stream);

/* ---- fir.Filter (dsp/filter/fir/filter.go:11-172) -------------------------
 * New(coeffs) for `channels` independent filters sharing the taps.
 * taps < 32: y[n] = sum_k h[k] x[n-k] (ProcessSample order, :46-69);
 * taps >= 32: the block path's reversed pairing y[n] = sum_j h[j] x[n-N+1+j]
 * (linear-buffer dot product, :74-159).  n == 0 taps: output untouched.     */
typedef struct ad_fir ad_fir;
int ad_fir_create(const double* coeffs, int64_t n_taps, int channels, int device, ad_fir** out);
int ad_fir_process_block(ad_fir* f, double* buf, int64_t n);                        /* :74-114 */
int ad_fir_process_block_to(ad_fir* f, double* dst, const double* src, int64_t n);  /* :119-159 */
int ad_fir_process_device(ad_fir* f, const double* d_src, int64_t src_stride, double* d_dst, int64_t dst_stride,
                          int64_t n, void* stream);
int ad_fir_reset(ad_fir* f); /* :162-172 */
void ad_fir_destroy(ad_fir* f);

/* ---- resample.Resampler (dsp/resample/resample.go:134-340) ----------------
 * Rational polyphase FIR sample-rate conversion, ratio up/down, for `channels`
 * independent streams that share the prototype and one scalar state (phase,
 * inputIndex, totalIn: every stream is fed the same block lengths).
 * create: NewRational (:153-187) with the prototype `taps` designed on the
 *   host (designPolyphaseFIR, resample_design.go:9-69); the ratio is reduced
 *   by its gcd, phase p is taps[p], taps[p+up], ..., so n_taps must be a
 *   positive multiple of the reduced up (T = n_taps/up taps per phase, a
 *   delay line of T-1 samples per channel).  up, down or channels <= 0, a
 *   reduced up or down above 2^30, such an n_taps, or a non-finite tap ->
 *   AD_ERR_INVALID_ARGUMENT, all before any device is touched.
 * predict_output_len: PredictOutputLen (:295-313) for the next call, in closed
 *   form: 0 for n_in <= 0 or L = totalIn + n_in - inputIndex <= 0, else
 *   ceil((L*up - phase) / down).
 * process: Process (:249-292).  Output j of a call is
 *   y = sum_k phases[(phase + j*down) % up][k] * x[inputIndex + (phase + j*down)/up - k],
 *   k ascending from y = 0, a rounded product and a rounded add per term (no
 *   FMA), bit for bit the reference's loop; samples before the stream start
 *   count as +0.  Host form: in [channels][n_in], out [channels][*n_out]
 *   packed at row length *n_out.  Device form: rows of n_in at in_stride and
 *   of *n_out at out_stride under the "Device buffers" contract above; only
 *   *n_out elements of each output row are written; input and output must not
 *   overlap (AD_ERR_INVALID_ARGUMENT).  out_cap is the room per output row:
 *   out_cap < the predicted length -> AD_ERR_INVALID_ARGUMENT with the state
 *   and the outputs untouched.  n_in == 0 does nothing; a call that yields
 *   *n_out == 0 (down > up and fewer samples than the next input index needs)
 *   writes nothing and still takes the samples in.  n_in must be < 2^31 and a
 *   call may produce at most 2^38 outputs; with the bounds on up and down
 *   every index product stays inside int64.
 * Calls on different streams are serialised through an event, as ad_fir's.
 * reset: Reset (:241-246), ordered after the last call.
 * kernel_info: the launch layout fixed at create -- outputs per tile, tiles a
 *   workgroup walks, whether the coefficient table and the input window are
 *   staged in LDS (else read from global memory), whether the next window is
 *   loaded while a tile computes, and the LDS bytes per workgroup.           */
typedef struct ad_resampler ad_resampler;
int ad_resampler_create(int64_t up, int64_t down, const double* taps, int64_t n_taps, int channels, int device,
                        ad_resampler** out);
int ad_resampler_predict_output_len(const ad_resampler* r, int64_t n_in, int64_t* n_out);
int ad_resampler_process(ad_resampler* r, const double* in, int64_t n_in, double* out, int64_t out_cap,
                         int64_t* n_out);
int ad_resampler_process_device(ad_resampler* r, const double* d_in, int64_t in_stride, int64_t n_in, double* d_out,
                                int64_t out_stride, int64_t out_cap, int64_t* n_out, void* stream);
int ad_resampler_reset(ad_resampler* r);
int ad_resampler_ratio(const ad_resampler* r, int64_t* up, int64_t* down); /* :316-318 */
int ad_resampler_taps_per_phase(const ad_resampler* r);                    /* :326-332 */
int ad_resampler_kernel_info(const ad_resampler* r, int* tile, int* tiles_per_workgroup, int* table_in_lds,
                             int* window_in_lds, int* window_prefetch, int64_t* lds_bytes);
void ad_resampler_destroy(ad_resampler* r);

/* ---- reverb.FDNReverb (dsp/effects/reverb/fdn_reverb.go:37-391) -------------
 * The modulated eight-line feedback delay network, for `channels` independent
 * instances that share one configuration (their samples and state differ).
 * ProcessSample (:199-241) bit for bit in its operation order -- every
 * product and sum rounded on its own, no FMA, the LFO phase the reference's
 * sequence of rounded additions and wraps -- except for the sine of the
 * modulation, which is the device math library's (within 1e-12 relative RMS
 * of the reference; with mod depth 0 the outputs are bit-identical).
 * default_config: NewFDNReverb's defaults (:12-19) at sample_rate.
 * validate: every setter's range (:95-186), host only: sample rate and RT60
 *   > 0, damp in [0, 1], the others >= 0, all finite; also refused: a
 *   configuration whose longest line would exceed 2^27 samples.
 * create: validation first (AD_ERR_INVALID_ARGUMENT), then the device
 *   (AD_ERR_NO_DEVICE without one).
 * set_param: the named setter with its side effects.  SAMPLE_RATE, PRE_DELAY
 *   and MOD_DEPTH run reconfigureDelays (:274-301): every damping state is
 *   zeroed, a line whose length changes (max(ceil(base_i*scale + depth) + 3, 4))
 *   is replaced by a zeroed one, the others keep their contents, the feedback
 *   gains are recomputed, the LFO phase stays.  RT60 recomputes the gains; WET,
 *   DRY, DAMP and MOD_RATE only store (they take effect with the next call).
 *   A rejected value changes nothing.  A reconfiguring setter waits for the
 *   handle's last call.
 * derived: the feedback gains pow(10, -3*delaySeconds/rt60) (:303-312), the
 *   lines' and the pre-delay line's buffer lengths, and the LFO phase after the
 *   last call (waits for it).  Any pointer may be NULL.
 * kernel_info: `block` = max(1, floor(1537 * sample_rate / 44100)) consecutive
 *   samples of a channel read none of each other's writes; the kernel walks a
 *   call in sub-blocks of `sub_block` <= block samples, `lds_bytes` of LDS each.
 * process: ProcessInPlace (:244-248) of every channel, any n >= 0; results do
 *   not depend on how a signal is cut into calls.  Host form: [channels][n].
 *   Device form: rows of n at `stride` under the "Device buffers" contract,
 *   asynchronous on `stream`; calls on different streams are serialised
 *   through an event, as ad_fir's.
 * reset: Reset (:189-197), ordered after the last call.                     */
typedef struct ad_fdn ad_fdn;
typedef struct ad_fdn_config {
  double sample_rate, wet, dry, rt60_seconds, damp, pre_delay_seconds, mod_depth_seconds, mod_rate_hz;
} ad_fdn_config;
#define AD_FDN_SAMPLE_RATE 0 /* SetSampleRate :95 */
#define AD_FDN_WET 1         /* SetWet :109 */
#define AD_FDN_DRY 2         /* SetDry :120 */
#define AD_FDN_RT60 3        /* SetRT60 :131 */
#define AD_FDN_DAMP 4        /* SetDamp :143 */
#define AD_FDN_PRE_DELAY 5   /* SetPreDelay :154 */
#define AD_FDN_MOD_DEPTH 6   /* SetModDepth :166 */
#define AD_FDN_MOD_RATE 7    /* SetModRate :178 */
void ad_fdn_default_config(ad_fdn_config* cfg, double sample_rate);
int ad_fdn_validate(const ad_fdn_config* cfg);
int ad_fdn_create(const ad_fdn_config* cfg, int channels, int device, ad_fdn** out);
int ad_fdn_set_param(ad_fdn* f, int which, double value);
int ad_fdn_get_config(const ad_fdn* f, ad_fdn_config* cfg);
int ad_fdn_derived(const ad_fdn* f, double feedback_gain[8], int64_t line_len[8], int64_t* pre_len,
                   double* lfo_phase);
int ad_fdn_kernel_info(const ad_fdn* f, int* block, int* sub_block, int* lds_bytes);
int ad_fdn_process(ad_fdn* f, double* buf, int64_t n);
int ad_fdn_process_device(ad_fdn* f, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_fdn_reset(ad_fdn* f);
void ad_fdn_destroy(ad_fdn* f);

/* ---- effects.Delay (dsp/effects/delay.go) and the graph's delay-simple
 * (dsp/effectchain/runtime_modulation.go:322-362) -----------------------------
 * The feedback delay with a linearly interpolated read and a one-pole ramp of
 * the delay time, for `channels` independent instances that share one
 * configuration.  ProcessSample (:140-166) bit for bit: the ramp, readExact,
 * floor, frac, the two-tap mix, the write-back and the output mix each rounded
 * as the reference rounds them, no FMA.  The rings ([channels][ceil(2 fs) + 1])
 * live in device memory.
 * config: mode 0 is Delay.  `smooth_coeff` 0 derives 1 - exp(-1/(fs * 0.010))
 *   (computeSmoothCoeff :255) with the host's exp; a caller whose exp differs
 *   in the last place (Go's math.Exp may) passes its own value, in (0, 1].
 *   get_config returns the coefficient in use.  mode 1 is delay-simple: only
 *   `delay_samples` (0 .. 2^27) counts, out[n] = in[n - delay_samples] copied,
 *   not computed (-0 and non-finite values pass unchanged); 0 leaves the
 *   buffer alone.
 * default_config: NewDelay's defaults (0.25 s, feedback 0.35, mix 0.25), mode 0.
 * validate: the setters' ranges (:63-128, :191-199), host only: sample rate
 *   > 0 and finite, time in [0.001, 2], feedback in [0, 0.99], mix in [0, 1];
 *   also refused: a ring of more than 2^27 samples.
 * create: validation, then the device (AD_ERR_NO_DEVICE without one).  Mode 0
 *   is NewDelay(sample_rate) followed by SetTargetTime(time_seconds),
 *   SetFeedback and SetMix, as the graph's configureDelay does: the delay
 *   starts at max(1, round(0.25 fs)) samples and ramps to round(time * fs).
 * set_param: SAMPLE_RATE is SetSampleRate (a ring whose length changes keeps
 *   its newest min(old, new) samples ending at write - 1, write becomes 0; the
 *   delay snaps to max(1, round(time * fs)); the coefficient is derived anew).
 *   TIME is SetTime (snaps, no clamp to one sample), TARGET_TIME is
 *   SetTargetTime (ramps), FEEDBACK and MIX store.  SMOOTH_COEFF replaces the
 *   coefficient (a caller's own exp, after SAMPLE_RATE).  SAMPLES (mode 1 only) is
 *   simpleDelayRuntime.Configure: another length is a zeroed ring.  A rejected
 *   value changes nothing.
 * derived: currentSamples after the last call, targetSamples, the ring's
 *   length as allocated (mode 1: delay_samples slots) and the write position.
 * kernel_info: `block` consecutive samples neither read each other's writes
 *   nor overwrite what another still reads, for the delay now and its target;
 *   `sub_block` is the persistent kernel's tile; `regime` and `launches` tell
 *   what the last call ran: 1 = one launch per block, 2 = one persistent
 *   launch (0 before the first call).  set_regime forces one (0: choose).
 * process / process_device / reset: as ad_fdn's.  Reset (:131-137) zeroes the
 *   rings and the write position and keeps currentSamples.                  */
typedef struct ad_delay ad_delay;
typedef struct ad_delay_config {
  double sample_rate, time_seconds, feedback, mix, smooth_coeff;
  int mode;              /* 0 Delay, 1 delay-simple */
  int64_t delay_samples; /* mode 1 */
} ad_delay_config;
#define AD_DELAY_SAMPLE_RATE 0 /* SetSampleRate :63 */
#define AD_DELAY_TIME 1        /* SetTime :77 */
#define AD_DELAY_FEEDBACK 2    /* SetFeedback :109 */
#define AD_DELAY_MIX 3         /* SetMix :120 */
#define AD_DELAY_TARGET_TIME 4 /* SetTargetTime :95 */
#define AD_DELAY_SAMPLES 5     /* mode 1: simpleDelayRuntime.Configure's delaySamples */
#define AD_DELAY_SMOOTH_COEFF 6 /* the ramp's coefficient, in (0, 1]; SAMPLE_RATE derives it anew */
void ad_delay_default_config(ad_delay_config* cfg, double sample_rate);
int ad_delay_validate(const ad_delay_config* cfg);
int ad_delay_create(const ad_delay_config* cfg, int channels, int device, ad_delay** out);
int ad_delay_set_param(ad_delay* d, int which, double value);
int ad_delay_get_config(const ad_delay* d, ad_delay_config* cfg);
int ad_delay_derived(const ad_delay* d, double* current_samples, double* target_samples, int64_t* ring_len,
                     int64_t* write_pos);
int ad_delay_kernel_info(const ad_delay* d, int* block, int* sub_block, int* regime, int* launches);
int ad_delay_set_regime(ad_delay* d, int regime);
int ad_delay_process(ad_delay* d, double* buf, int64_t n);
int ad_delay_process_device(ad_delay* d, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_delay_reset(ad_delay* d);
void ad_delay_destroy(ad_delay* d);

/* ---- modulation.Flanger (dsp/effects/modulation/flanger.go) -----------------
 * The LFO-modulated Hermite delay with signed feedback, for `channels`
 * instances sharing one configuration.  Process (:259-282) bit for bit in its
 * operation order except for the sine of the LFO, which is the device math
 * library's (with depth 0 the outputs are bit-identical); the LFO phase is
 * the reference's sequence of rounded additions and wraps.  A channel's ring
 * (max(ceil((base + depth) fs) + 3, 4) samples) is held in LDS during a call.
 * default_config: defaultFlangerConfig (:9-13) at sample_rate.
 * validate: validateParams (:317-350), host only, `base + depth > 0.01`
 *   included; also refused: a ring of more than 4065 samples (sample rates
 *   above about 400 kHz).
 * set_param: the named setter; SAMPLE_RATE, DEPTH and BASE_DELAY run
 *   reconfigureDelayLine (:352-390): a ring whose length changes keeps its
 *   newest min(old, new) samples, write becomes 0, the phase stays.  A rejected
 *   value changes nothing (the setters' rollbacks :187-224).
 * derived: ring length, maxDelay, write position, and the LFO phase after the
 *   last call (waits for it).  kernel_info: `block` = max(1, P - 1),
 *   P = floor(max(1, base * fs)), consecutive samples read none of each other's
 *   writes; a wave is a tile of 64 / sub_block channels x sub_block samples.
 * process / process_device / reset: as ad_fdn's.  Reset (:249-256) also
 *   zeroes the phase.                                                       */
typedef struct ad_flanger ad_flanger;
typedef struct ad_flanger_config {
  double sample_rate, rate_hz, depth_seconds, base_delay_seconds, feedback, mix;
} ad_flanger_config;
#define AD_FLANGER_SAMPLE_RATE 0 /* SetSampleRate :165 */
#define AD_FLANGER_RATE 1        /* SetRateHz :176 */
#define AD_FLANGER_DEPTH 2       /* SetDepthSeconds :187 */
#define AD_FLANGER_BASE_DELAY 3  /* SetBaseDelaySeconds :206 */
#define AD_FLANGER_FEEDBACK 4    /* SetFeedback :227 */
#define AD_FLANGER_MIX 5         /* SetMix :238 */
void ad_flanger_default_config(ad_flanger_config* cfg, double sample_rate);
int ad_flanger_validate(const ad_flanger_config* cfg);
int ad_flanger_create(const ad_flanger_config* cfg, int channels, int device, ad_flanger** out);
int ad_flanger_set_param(ad_flanger* f, int which, double value);
int ad_flanger_get_config(const ad_flanger* f, ad_flanger_config* cfg);
int ad_flanger_derived(const ad_flanger* f, int64_t* ring_len, int64_t* max_delay, int64_t* write_pos,
                       double* lfo_phase);
int ad_flanger_kernel_info(const ad_flanger* f, int* block, int* sub_block, int* channels_per_workgroup,
                           int* lds_bytes);
int ad_flanger_process(ad_flanger* f, double* buf, int64_t n);
int ad_flanger_process_device(ad_flanger* f, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_flanger_reset(ad_flanger* f);
void ad_flanger_destroy(ad_flanger* f);

/* ---- modulation.Phaser, Tremolo, RingModulator (dsp/effects/modulation/
 * phaser.go, tremolo.go, ring_modulator.go) ----------------------------------
 * For `channels` instances sharing one configuration.  The LFO (carrier) phase
 * is one sequence for every channel: a call steps it on the host, the
 * reference's rounded additions and wraps bit for bit, and the kernels take the
 * sine once per sample.  Given that per-sample table (the phaser's allpass
 * coefficient, the tremolo's gain currentMod, the ring modulator's carrier),
 * Process is bit for bit the reference's operation order; the table itself
 * differs from the reference by the device math library's sin and tan only
 * (and is exact where it does not depend on them: tremolo depth 0).
 * A config's field k is parameter k.
 * default_config: the reference's defaults at sample_rate.
 * validate: validateParams, host only.  Phaser: max_freq_hz < 0.49 sample_rate
 *   strictly, stages in [1, 12].  Tremolo: smoothing_coeff is 0 (derive
 *   1 - exp(-1 / ((ms / 1000) fs)) clamped to [0, 1] with the C library's exp, 1
 *   for smoothing <= 0) or a caller's own coefficient in (0, 1].
 * set_param: the named setter with its own check; a rejected value changes
 *   nothing (the reference's phaser keeps a rejected sample rate or range; this
 *   handle does not).  AD_PHASER_MIN_FREQ / MAX_FREQ are SetFrequencyRangeHz
 *   with the other bound as it is, ad_phaser_set_range sets both at once.
 *   AD_PHASER_STAGES: the same count keeps the stage states, another one zeroes
 *   them and keeps the feedback sample and the phase (SetStages :221-233).
 *   Tremolo SAMPLE_RATE and SMOOTHING derive the coefficient anew;
 *   get_config reports the coefficient in use.  Ring modulator SAMPLE_RATE and
 *   CARRIER recompute the stored increment 2 pi carrier / fs.
 * peek_lfo: the phases of the next n samples and the table values the kernels
 *   would use for them (host arrays [n]), by the device code a call runs;
 *   nothing advances.  phase_out[0] is the handle's phase state.
 * kernel_info: phaser: channels per workgroup (one per lane), samples staged
 *   through LDS per chunk, LDS bytes.  Tremolo: samples of a row a workgroup
 *   of the apply kernel covers, the stepper lane's chunk, whether the gain is
 *   smoothed (coefficient < 1).  Ring modulator: the same first value, the
 *   table kernel's threads, the stored phase increment.
 * process / process_device / reset: as ad_fdn's.  Reset: phaser :258-265
 *   (stages, feedback sample, phase), tremolo :195-198 (phase 0, gain 1), ring
 *   modulator :138-140 (phase).                                              */
typedef struct ad_phaser ad_phaser;
typedef struct ad_phaser_config {
  double sample_rate, rate_hz, min_freq_hz, max_freq_hz, feedback, mix;
  int stages;
} ad_phaser_config;
#define AD_PHASER_SAMPLE_RATE 0 /* SetSampleRate :183 */
#define AD_PHASER_RATE 1        /* SetRateHz :194 */
#define AD_PHASER_MIN_FREQ 2    /* SetFrequencyRangeHz :205 */
#define AD_PHASER_MAX_FREQ 3
#define AD_PHASER_FEEDBACK 4    /* SetFeedback :236 */
#define AD_PHASER_MIX 5         /* SetMix :247 */
#define AD_PHASER_STAGES 6      /* SetStages :221 */
void ad_phaser_default_config(ad_phaser_config* cfg, double sample_rate);
int ad_phaser_validate(const ad_phaser_config* cfg);
int ad_phaser_create(const ad_phaser_config* cfg, int channels, int device, ad_phaser** out);
int ad_phaser_set_param(ad_phaser* p, int which, double value);
int ad_phaser_set_range(ad_phaser* p, double min_freq_hz, double max_freq_hz);
int ad_phaser_get_config(const ad_phaser* p, ad_phaser_config* cfg);
int ad_phaser_kernel_info(const ad_phaser* p, int* channels_per_workgroup, int* tile, int* lds_bytes);
int ad_phaser_peek_lfo(ad_phaser* p, int64_t n, double* phase_out, double* coef_out);
int ad_phaser_process(ad_phaser* p, double* buf, int64_t n);
int ad_phaser_process_device(ad_phaser* p, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_phaser_reset(ad_phaser* p);
void ad_phaser_destroy(ad_phaser* p);

typedef struct ad_tremolo ad_tremolo;
typedef struct ad_tremolo_config {
  double sample_rate, rate_hz, depth, smoothing_ms, mix, smoothing_coeff;
} ad_tremolo_config;
#define AD_TREMOLO_SAMPLE_RATE 0     /* SetSampleRate :138 */
#define AD_TREMOLO_RATE 1            /* SetRateHz :150 */
#define AD_TREMOLO_DEPTH 2           /* SetDepth :161 */
#define AD_TREMOLO_SMOOTHING 3       /* SetSmoothingMs :172 */
#define AD_TREMOLO_MIX 4             /* SetMix :184 */
#define AD_TREMOLO_SMOOTHING_COEFF 5 /* smoothingCoef, in (0, 1]; SAMPLE_RATE and SMOOTHING derive it anew */
void ad_tremolo_default_config(ad_tremolo_config* cfg, double sample_rate);
int ad_tremolo_validate(const ad_tremolo_config* cfg);
int ad_tremolo_create(const ad_tremolo_config* cfg, int channels, int device, ad_tremolo** out);
int ad_tremolo_set_param(ad_tremolo* t, int which, double value);
int ad_tremolo_get_config(const ad_tremolo* t, ad_tremolo_config* cfg);
int ad_tremolo_kernel_info(const ad_tremolo* t, int* samples_per_workgroup, int* smooth_chunk, int* smoothed);
int ad_tremolo_peek_lfo(ad_tremolo* t, int64_t n, double* phase_out, double* gain_out);
int ad_tremolo_process(ad_tremolo* t, double* buf, int64_t n);
int ad_tremolo_process_device(ad_tremolo* t, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_tremolo_reset(ad_tremolo* t);
void ad_tremolo_destroy(ad_tremolo* t);

typedef struct ad_ringmod ad_ringmod;
typedef struct ad_ringmod_config {
  double sample_rate, carrier_hz, mix;
} ad_ringmod_config;
#define AD_RINGMOD_SAMPLE_RATE 0 /* SetSampleRate :103 */
#define AD_RINGMOD_CARRIER 1     /* SetCarrierHz :115 */
#define AD_RINGMOD_MIX 2         /* SetMix :127 */
void ad_ringmod_default_config(ad_ringmod_config* cfg, double sample_rate);
int ad_ringmod_validate(const ad_ringmod_config* cfg);
int ad_ringmod_create(const ad_ringmod_config* cfg, int channels, int device, ad_ringmod** out);
int ad_ringmod_set_param(ad_ringmod* r, int which, double value);
int ad_ringmod_get_config(const ad_ringmod* r, ad_ringmod_config* cfg);
int ad_ringmod_kernel_info(const ad_ringmod* r, int* samples_per_workgroup, int* table_threads, double* phase_inc);
int ad_ringmod_peek_lfo(ad_ringmod* r, int64_t n, double* phase_out, double* carrier_out);
int ad_ringmod_process(ad_ringmod* r, double* buf, int64_t n);
int ad_ringmod_process_device(ad_ringmod* r, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_ringmod_reset(ad_ringmod* r);
void ad_ringmod_destroy(ad_ringmod* r);

/* ---- effects.Distortion, effects.BitCrusher (dsp/effects/distortion.go,
 * bit_crusher.go) -------------------------------------------------------------
 * For `channels` instances sharing one configuration.  Both are time-parallel:
 * the distortion is pointwise (its Chebyshev DC bypass, a one-pole recurrence
 * per channel, is the one serial path), the bit crusher is a sample-and-hold
 * whose update positions follow from a counter that is the same for every
 * channel, kept on the host.  Every expression is evaluated in the reference's
 * written order, each operation rounded on its own, the clamps as the two
 * comparisons the reference writes (a NaN passes them and is zeroed by the
 * finite check).  So the modes made of + - * / (SoftClip, HardClip,
 * Waveshaper1-4 and 6, Saturate, Saturate2, Chebyshev; with the polynomial
 * approximation also Tanh, Waveshaper7 and SoftSat) and the bit crusher are
 * bit for bit the reference's; the exact Tanh, Waveshaper5, 7, 8 and SoftSat
 * differ from it by the device math library's tanh, atan and exp only, and
 * Process is bit for bit in (1 - mix) + curve mix given ad_distortion_curve.
 * Constants the reference recomputes per sample are computed once on the host
 * with the C library: atan(1 + 4 shape), 1 + 6 shape, 1 + 2 shape, 1 - mix,
 * quantLevels = exp2(bitDepth - 1).
 * ad_distortion_config: field k (0..7) is parameter k; mode is DistortionMode
 *   (distortion.go:36-52, 0..14), approx 0 exact / 1 polynomial, cheb_harmonic
 *   0 all / 1 odd / 2 even, cheb_invert and cheb_dc_bypass 0 or 1.
 * validate: the setters' own ranges (distortion.go:364-529, bit_crusher.go:
 *   137-183) and validateChebyshevParity, host only.
 * set_param: the named setter with its own check; the int parameters take a
 *   whole number.  A rejected value changes nothing: the reference's
 *   SetChebyshevOrder and SetChebyshevHarmonicMode keep a value that fails the
 *   parity rule; these handles do not.  No setter clears state.
 * ad_distortion_set_weights: SetChebyshevWeights :514-529, n <= 16 finite
 *   values, the other slots zeroed.  Weights are active when one of the first
 *   cheb_order slots is nonzero (:690-695).
 * ad_distortion_curve: wet[i] = shapeSample(x[i]) * outputLevel, 0 where that
 *   is not finite, for host arrays [n], by the device code a call runs (x is
 *   the shaper's argument, after bias and drive).  Nothing advances.
 * derived: the host-computed constants above and whether weights are active;
 *   bit crusher: quantLevels, holdCounter and holdValue of `channel`.
 * kernel_info: distortion: samples of a row a workgroup of the pointwise
 *   kernel covers; channels per workgroup, samples staged per chunk and LDS
 *   bytes of the DC-bypass kernel.  Bit crusher: samples of a row a workgroup
 *   covers, the span of whole hold periods it stages (0 at downsample 1), its
 *   LDS bytes.
 * process / process_device / reset: as ad_fdn's.  Reset: distortion :532-535
 *   (the two DC states), bit crusher :186-189 (counter 0, hold 0).           */
typedef struct ad_distortion ad_distortion;
typedef struct ad_distortion_config {
  double sample_rate, drive, mix, output_level, clip_level, shape, bias, cheb_gain, cheb_weights[16];
  int mode, approx, cheb_order, cheb_harmonic, cheb_invert, cheb_dc_bypass;
} ad_distortion_config;
#define AD_DISTORTION_SAMPLE_RATE 0     /* SetSampleRate :365 */
#define AD_DISTORTION_DRIVE 1           /* SetDrive :398 */
#define AD_DISTORTION_MIX 2             /* SetMix :409 */
#define AD_DISTORTION_OUTPUT_LEVEL 3    /* SetOutputLevel :420 */
#define AD_DISTORTION_CLIP_LEVEL 4      /* SetClipLevel :432 */
#define AD_DISTORTION_SHAPE 5           /* SetShape :444 */
#define AD_DISTORTION_BIAS 6            /* SetBias :455 */
#define AD_DISTORTION_CHEB_GAIN 7       /* SetChebyshevGainLevel :493 */
#define AD_DISTORTION_MODE 8            /* SetMode :376 */
#define AD_DISTORTION_APPROX 9          /* SetApproxMode :387 */
#define AD_DISTORTION_CHEB_ORDER 10     /* SetChebyshevOrder :466 */
#define AD_DISTORTION_CHEB_HARMONIC 11  /* SetChebyshevHarmonicMode :477 */
#define AD_DISTORTION_CHEB_INVERT 12    /* SetChebyshevInvert :488 */
#define AD_DISTORTION_CHEB_DC_BYPASS 13 /* SetChebyshevDCBypass :505 */
void ad_distortion_default_config(ad_distortion_config* cfg, double sample_rate);
int ad_distortion_validate(const ad_distortion_config* cfg);
int ad_distortion_create(const ad_distortion_config* cfg, int channels, int device, ad_distortion** out);
int ad_distortion_set_param(ad_distortion* d, int which, double value);
int ad_distortion_set_weights(ad_distortion* d, const double* w, int n);
int ad_distortion_get_config(const ad_distortion* d, ad_distortion_config* cfg);
int ad_distortion_derived(const ad_distortion* d, double* atan_scale, double* scale6, double* scale2,
                          double* one_minus_mix, int* weights_active);
int ad_distortion_kernel_info(const ad_distortion* d, int* samples_per_workgroup, int* dc_channels_per_workgroup,
                              int* dc_tile, int* dc_lds_bytes);
int ad_distortion_curve(ad_distortion* d, const double* x, int64_t n, double* wet);
int ad_distortion_process(ad_distortion* d, double* buf, int64_t n);
int ad_distortion_process_device(ad_distortion* d, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_distortion_reset(ad_distortion* d);
void ad_distortion_destroy(ad_distortion* d);

typedef struct ad_bitcrusher ad_bitcrusher;
typedef struct ad_bitcrusher_config {
  double sample_rate, bit_depth, mix;
  int downsample;
} ad_bitcrusher_config;
#define AD_BITCRUSHER_SAMPLE_RATE 0 /* SetSampleRate :138 */
#define AD_BITCRUSHER_BIT_DEPTH 1   /* SetBitDepth :149 */
#define AD_BITCRUSHER_MIX 2         /* SetMix :175 */
#define AD_BITCRUSHER_DOWNSAMPLE 3  /* SetDownsample :163 */
void ad_bitcrusher_default_config(ad_bitcrusher_config* cfg, double sample_rate);
int ad_bitcrusher_validate(const ad_bitcrusher_config* cfg);
int ad_bitcrusher_create(const ad_bitcrusher_config* cfg, int channels, int device, ad_bitcrusher** out);
int ad_bitcrusher_set_param(ad_bitcrusher* b, int which, double value);
int ad_bitcrusher_get_config(const ad_bitcrusher* b, ad_bitcrusher_config* cfg);
int ad_bitcrusher_derived(ad_bitcrusher* b, int channel, double* quant_levels, int* counter, double* hold_value);
int ad_bitcrusher_kernel_info(const ad_bitcrusher* b, int* samples_per_workgroup, int* span, int* lds_bytes);
int ad_bitcrusher_process(ad_bitcrusher* b, double* buf, int64_t n);
int ad_bitcrusher_process_device(ad_bitcrusher* b, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_bitcrusher_reset(ad_bitcrusher* b);
void ad_bitcrusher_destroy(ad_bitcrusher* b);

/* ---- dynamics.TransientShaper, dynamics.DeEsser (dsp/effects/dynamics/
 * transient_shaper.go, deesser.go) --------------------------------------------
 * For `channels` instances sharing one configuration.  In both only the
 * envelope (in the de-esser behind its detection cascade) is serial in time;
 * it runs one channel per lane in the reference's own operations and branch
 * forms, so the envelope, the transient shaper's output and the de-esser's
 * listen output are bit for bit the reference's.  Everything after env[t] is a
 * pointwise pass.  The de-esser's gain (calculateGain :513-557) differs from
 * the reference by the device math library's log and exp2 only, and Process is
 * bit for bit the reference's given ad_deesser_gain.
 * config: a *_coeff of 0 means "derive it with the C library's exp"
 *   (timeMsToCoeff transient_shaper.go:184-200, updateTimeConstants
 *   deesser.go:573-576); another value is the caller's own, for a caller whose
 *   exp is not the C library's.  get_config reports the coefficients in use.
 *   De-esser: mode 0 split band / 1 wideband, detector 0 bandpass / 1 highpass,
 *   listen 0 / 1, filter_order 1..4.
 * validate: the setters' own ranges (transient_shaper.go:14-19, 57-117;
 *   deesser.go:57-72, 228-409), the de-esser's frequency below fs / 2 (:235,
 *   :399); host only.
 * set_param: the named setter with its own check; the int parameters take a
 *   whole number.  A rejected value changes nothing.  The setters that end in
 *   updateCoefficients / updateTimeConstants derive both envelope coefficients
 *   again, as the reference does.  De-esser SAMPLE_RATE, FREQ, Q, DETECTOR and
 *   FILTER_ORDER run rebuildFilters :578-622: both cascades' states are zeroed,
 *   the envelope and the metrics stay.
 * derived: on a config, host only, no device needed: the coefficients in use;
 *   de-esser also section[5] = {b0, b1, b2, a1, a2} of every stage of both
 *   cascades, bandNorm, thresholdLog2, kneeWidthLog2, rangeLin.
 * kernel_info: channels per workgroup, samples staged per chunk and LDS bytes
 *   of the walk the next call runs; de-esser: the cascades it walks.  One
 *   stands for both while their states are equal; a listen or wideband call
 *   advances detectFilters alone, after which split-band calls walk two until
 *   a rebuild or Reset.
 * get_state / set_state: one channel's envelope; de-esser: also detect[4][2]
 *   and band[4][2], {d0, d1} of each section.
 * ad_deesser_metrics: GetMetrics :499 of `channel`; reset_metrics :504.
 * ad_deesser_gain: gains[i] = calculateGain(levels[i]) for host arrays [n], by
 *   the device code a call runs.  Nothing advances.
 * process / process_device / reset: as ad_fdn's.  Reset: transient shaper
 *   :135-137 (the envelope), de-esser :485-496 (envelope, cascades, metrics). */
typedef struct ad_transient ad_transient;
typedef struct ad_transient_config {
  double sample_rate, attack_amount, sustain_amount, attack_ms, release_ms, attack_coeff, release_coeff;
} ad_transient_config;
#define AD_TRANSIENT_SAMPLE_RATE 0    /* SetSampleRate transient_shaper.go:107 */
#define AD_TRANSIENT_ATTACK_AMOUNT 1  /* SetAttackAmount transient_shaper.go:57 */
#define AD_TRANSIENT_SUSTAIN_AMOUNT 2 /* SetSustainAmount transient_shaper.go:69 */
#define AD_TRANSIENT_ATTACK 3         /* SetAttack transient_shaper.go:81 */
#define AD_TRANSIENT_RELEASE 4        /* SetRelease transient_shaper.go:94 */
#define AD_TRANSIENT_ATTACK_COEFF 5   /* attackCoeff, a caller's own */
#define AD_TRANSIENT_RELEASE_COEFF 6  /* releaseCoeff, a caller's own */
void ad_transient_default_config(ad_transient_config* cfg, double sample_rate);
int ad_transient_validate(const ad_transient_config* cfg);
int ad_transient_derived(const ad_transient_config* cfg, double* attack_coeff, double* release_coeff);
int ad_transient_create(const ad_transient_config* cfg, int channels, int device, ad_transient** out);
int ad_transient_set_param(ad_transient* t, int which, double value);
int ad_transient_get_config(const ad_transient* t, ad_transient_config* cfg);
int ad_transient_kernel_info(const ad_transient* t, int* channels_per_workgroup, int* tile, int* lds_bytes);
int ad_transient_get_state(ad_transient* t, int channel, double* envelope);
int ad_transient_set_state(ad_transient* t, int channel, double envelope);
int ad_transient_process(ad_transient* t, double* buf, int64_t n);
int ad_transient_process_device(ad_transient* t, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_transient_reset(ad_transient* t);
void ad_transient_destroy(ad_transient* t);

typedef struct ad_deesser ad_deesser;
typedef struct ad_deesser_config {
  double sample_rate, freq_hz, q, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db, attack_coeff,
      release_coeff;
  int mode, detector, listen, filter_order;
} ad_deesser_config;
#define AD_DEESSER_SAMPLE_RATE 0   /* SetSampleRate deesser.go:394 */
#define AD_DEESSER_FREQ 1          /* SetFrequency deesser.go:228 */
#define AD_DEESSER_Q 2             /* SetQ deesser.go:248 */
#define AD_DEESSER_THRESHOLD 3     /* SetThreshold deesser.go:263 */
#define AD_DEESSER_RATIO 4         /* SetRatio deesser.go:276 */
#define AD_DEESSER_KNEE 5          /* SetKnee deesser.go:291 */
#define AD_DEESSER_ATTACK 6        /* SetAttack deesser.go:306 */
#define AD_DEESSER_RELEASE 7       /* SetRelease deesser.go:321 */
#define AD_DEESSER_RANGE 8         /* SetRange deesser.go:336 */
#define AD_DEESSER_ATTACK_COEFF 9  /* attackCoeff, a caller's own */
#define AD_DEESSER_RELEASE_COEFF 10 /* releaseCoeff, a caller's own */
#define AD_DEESSER_MODE 11         /* SetMode deesser.go:350 */
#define AD_DEESSER_DETECTOR 12     /* SetDetector deesser.go:361 */
#define AD_DEESSER_LISTEN 13       /* SetListen deesser.go:375 */
#define AD_DEESSER_FILTER_ORDER 14 /* SetFilterOrder deesser.go:381 */
void ad_deesser_default_config(ad_deesser_config* cfg, double sample_rate);
int ad_deesser_validate(const ad_deesser_config* cfg);
int ad_deesser_derived(const ad_deesser_config* cfg, double* section, double* band_norm, double* threshold_log2,
                       double* knee_width_log2, double* range_lin, double* attack_coeff, double* release_coeff);
int ad_deesser_create(const ad_deesser_config* cfg, int channels, int device, ad_deesser** out);
int ad_deesser_set_param(ad_deesser* d, int which, double value);
int ad_deesser_get_config(const ad_deesser* d, ad_deesser_config* cfg);
int ad_deesser_kernel_info(const ad_deesser* d, int* channels_per_workgroup, int* tile, int* lds_bytes, int* cascades);
int ad_deesser_get_state(ad_deesser* d, int channel, double* envelope, double* detect, double* band);
int ad_deesser_set_state(ad_deesser* d, int channel, double envelope, const double* detect, const double* band);
int ad_deesser_metrics(ad_deesser* d, int channel, double* detection_level, double* gain_reduction);
int ad_deesser_reset_metrics(ad_deesser* d);
int ad_deesser_gain(ad_deesser* d, const double* levels, double* gains, int64_t n);
int ad_deesser_process(ad_deesser* d, double* buf, int64_t n);
int ad_deesser_process_device(ad_deesser* d, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_deesser_reset(ad_deesser* d);
void ad_deesser_destroy(ad_deesser* d);

/* ---- effects.Vocoder (dsp/effects/vocoder.go) --------------------------------
 * For `channels` instances sharing one configuration; each channel has its
 * own modulator row, carrier row and state.  One channel is up to 32 band
 * recurrences whose products are summed per sample, so a channel is walked by
 * one wave with a band per lane: lanes 0..31 carry the modulator side of band
 * b (analysis section and envelope; with downsampling the group's anti-alias
 * section, then the decimated analysis section and envelope on the group's
 * ticks), lanes 32..63 the carrier side (synthesis section).  A second phase
 * forms the band-order sum and the mix, one sample per lane.  Every product
 * and sum is rounded on its own (no FMA): a call is bit for bit ProcessBlock
 * :634-645 given the tables of ad_vocoder_derived, which come from the C
 * library's cos, sin and exp in the reference's operation order.
 * config: layout 0 ThirdOctave / 1 Bark (:15-25); synth_q is used by
 *   ThirdOctave always and by Bark only when synth_q_set (:381-384);
 *   downsample 0 / 1 (WithDownsampling :90).
 * validate: the options' own ranges (:49-56, :98-193), the sample rate
 *   positive and finite, and at least one usable band (:320, :361); host only.
 * set_param: the named setter with its own check.  SAMPLE_RATE (:673-683)
 *   clears the envelopes and every section's state (and the counter when
 *   downsampling is on); a rate that leaves no usable band is refused and
 *   changes nothing (the reference leaves a broken instance behind).
 *   DOWNSAMPLING (:737-769) takes 0 or 1: on, it rebuilds the decimated
 *   analysis sections, the anti-alias sections and the counter, also when it
 *   was on already, and keeps the envelopes and the full-rate sections; off,
 *   it zeroes the counter.  The layout and the synthesis Q have no setter in
 *   the reference and none here.
 * process: host rows [channels][n] each; out may be modulator or carrier.
 * process_device: device rows [channels][stride]; out may be exactly the
 *   modulator's or the carrier's rows (same pointer and stride) or rows that
 *   overlap neither; asynchronous on `stream`.
 * reset: Reset :648-670. */
#define AD_VOCODER_MAX_BANDS 32
typedef struct ad_vocoder ad_vocoder;
typedef struct ad_vocoder_config {
  double sample_rate, synth_q, attack_ms, release_ms, input_level, synth_level, vocoder_level;
  int downsample, layout, synth_q_set;
} ad_vocoder_config;
#define AD_VOCODER_SAMPLE_RATE 0   /* SetSampleRate vocoder.go:673 */
#define AD_VOCODER_ATTACK 2        /* SetAttack vocoder.go:772 */
#define AD_VOCODER_RELEASE 3       /* SetRelease vocoder.go:786 */
#define AD_VOCODER_INPUT_LEVEL 4   /* SetInputLevel vocoder.go:800 */
#define AD_VOCODER_SYNTH_LEVEL 5   /* SetSynthLevel vocoder.go:812 */
#define AD_VOCODER_VOCODER_LEVEL 6 /* SetVocoderLevel vocoder.go:824 */
#define AD_VOCODER_DOWNSAMPLING 7  /* SetDownsampling vocoder.go:737 */
/* What the reference caches for a config: sections are {b0, b1, b2, a1, a2}.  With downsampling off num_groups
 * and downsample_max are 0 and the decimation entries are zero. */
typedef struct ad_vocoder_tables {
  int num_bands, num_groups, downsample_max;
  int factors[AD_VOCODER_MAX_BANDS];       /* downsampleFactors, by band */
  int group_of_band[AD_VOCODER_MAX_BANDS]; /* index into group_factors */
  int group_factors[AD_VOCODER_MAX_BANDS]; /* downsampleGroupFactors, ascending */
  double analysis[AD_VOCODER_MAX_BANDS][5], synthesis[AD_VOCODER_MAX_BANDS][5];
  double decimated[AD_VOCODER_MAX_BANDS][5]; /* downsampleAnalysisFilters, by band */
  double antialias[AD_VOCODER_MAX_BANDS][5]; /* downsampleGroupAAFilters, by group */
  double attack_coeff, release_coeff;
  double ds_attack[AD_VOCODER_MAX_BANDS], ds_release[AD_VOCODER_MAX_BANDS];
} ad_vocoder_tables;
void ad_vocoder_default_config(ad_vocoder_config* cfg, double sample_rate);
int ad_vocoder_validate(const ad_vocoder_config* cfg);
int ad_vocoder_derived(const ad_vocoder_config* cfg, ad_vocoder_tables* out);
int ad_vocoder_create(const ad_vocoder_config* cfg, int channels, int device, ad_vocoder** out);
int ad_vocoder_set_param(ad_vocoder* v, int which, double value);
int ad_vocoder_get_config(const ad_vocoder* v, ad_vocoder_config* cfg);
int ad_vocoder_num_bands(const ad_vocoder* v, int* num_bands);
/* DownsampleFactors :722-731: *count = 0 with downsampling off, else NumBands factors into factors[cap]. */
int ad_vocoder_downsample_factors(const ad_vocoder* v, int* factors, int cap, int* count);
int ad_vocoder_kernel_info(const ad_vocoder* v, int* lanes_per_channel, int* tile, int* lds_bytes);
/* One channel's state: {analysis s0, s1, synthesis s0, s1, decimated s0, s1, envelope} by band, then the
 * anti-alias {s0, s1} by group: state[9][AD_VOCODER_MAX_BANDS]; *counter: downsampleCount. */
int ad_vocoder_get_state(ad_vocoder* v, int channel, double* state, int* counter);
int ad_vocoder_process(ad_vocoder* v, const double* modulator, const double* carrier, double* out, int64_t n);
int ad_vocoder_process_device(ad_vocoder* v, const double* d_modulator, int64_t modulator_stride,
                              const double* d_carrier, int64_t carrier_stride, double* d_out, int64_t out_stride,
                              int64_t n, void* stream);
int ad_vocoder_reset(ad_vocoder* v);
void ad_vocoder_destroy(ad_vocoder* v);

/* ---- dynamics.LookaheadLimiter (dsp/effects/dynamics/lookahead_limiter.go) ----
 * For `channels` instances sharing one configuration.  The limiter is a
 * Compressor core fixed at ratio 100, attack 0.1 ms, knee 0 and no makeup
 * (:42-70), feed-forward with the peak detector.  Its gain comes from the
 * sidechain sample (core.ProcessSample(0, sidechain) :197) and multiplies the
 * program delayed by D = round(lookahead_ms * sample_rate / 1000) samples,
 * halves away from zero as math.Round.  A call is three passes: the envelope
 * of |sidechain| (serial in time, one channel per lane, the de-esser's walk),
 * a copy of the call's program samples, and a pointwise pass that writes
 * gain(env[t]) * program[t - D] in place, the first D samples from a
 * per-channel history of the calls before.  The copy is what makes in place
 * safe: no thread reads a program sample another one writes.
 * The envelope, the delayed samples and the product are bit for bit the
 * reference's; the gain (GainForLevel core.go:288-309) differs from it by the
 * device math library's log and exp2 only, as the de-esser's.
 * set_param: the named setter with its own range (:8-19, :98-161).  LOOKAHEAD
 *   and SAMPLE_RATE rebuild the delay line zeroed, also when the value is
 *   unchanged (rebuildDelayBuffer :232-239); the envelope stays.
 * process / process_device: the program rows in place; sidechain NULL: the
 *   program is its own detector (ProcessInPlace :213); else rows of
 *   sidechain_n samples, read as 0 from there on (ProcessInPlaceSidechain
 *   :221-230), which must not overlap the program rows.
 * ad_lookahead_gain: gains[i] = GainForLevel(levels[i]) for host arrays, by
 *   the device code a call runs.  Nothing advances.
 * ad_lookahead_last_envelope: the detector envelope of every sample of the
 *   last call, [channels][n] with n that call's length (a call short enough
 *   for one pass; else AD_ERR_INVALID_ARGUMENT).
 * reset: Reset :176-183: the envelope and the delay line. */
typedef struct ad_lookahead ad_lookahead;
typedef struct ad_lookahead_config {
  double sample_rate, threshold_db, release_ms, lookahead_ms;
} ad_lookahead_config;
#define AD_LOOKAHEAD_SAMPLE_RATE 0 /* SetSampleRate lookahead_limiter.go:146 */
#define AD_LOOKAHEAD_THRESHOLD 1   /* SetThreshold :99 */
#define AD_LOOKAHEAD_RELEASE 2     /* SetRelease :116 */
#define AD_LOOKAHEAD_LOOKAHEAD 3   /* SetLookahead :133 */
void ad_lookahead_default_config(ad_lookahead_config* cfg, double sample_rate);
int ad_lookahead_validate(const ad_lookahead_config* cfg);
int ad_lookahead_derived(const ad_lookahead_config* cfg, double* attack_coeff, double* release_coeff,
                         double* threshold_log2, int64_t* delay_samples);
int ad_lookahead_create(const ad_lookahead_config* cfg, int channels, int device, ad_lookahead** out);
int ad_lookahead_set_param(ad_lookahead* l, int which, double value);
int ad_lookahead_get_config(const ad_lookahead* l, ad_lookahead_config* cfg);
int ad_lookahead_get_state(ad_lookahead* l, int channel, double* envelope);
int ad_lookahead_gain(ad_lookahead* l, const double* levels, double* gains, int64_t n);
int ad_lookahead_last_envelope(ad_lookahead* l, double* envelope, int64_t n);
int ad_lookahead_process(ad_lookahead* l, double* program, const double* sidechain, int64_t sidechain_n, int64_t n);
int ad_lookahead_process_device(ad_lookahead* l, double* d_program, int64_t stride, const double* d_sidechain,
                                int64_t sidechain_stride, int64_t sidechain_n, int64_t n, void* stream);
int ad_lookahead_reset(ad_lookahead* l);
void ad_lookahead_destroy(ad_lookahead* l);

/* The graph nodes with a second input (chain_process.go:124-175, 226-259): cfg[i] of an AD_FXN_LOOKAHEAD or
 * AD_FXN_VOCODER node.  The node's `parents` are its main parents (the edges whose toPortIndex is not 1) and mix
 * into its buffer as every node's do; side_parents are the edges with toPortIndex 1, in edge order, and mix the
 * same way (a copy for one, the edge-order sum times 1/k for more) into the side input: the limiter's detector,
 * the vocoder's carrier (runtime_misc.go:122-124).  side_ports[k] 1: the high band of a split-freq parent.
 * n_side 0: the side input is the node's own mixed input.  A bypassed node mixes its main parents only.  Unlike
 * the reference, whose splitMainAndSideParents filters the node's incoming list in place and so loses a side
 * edge listed before a main edge from the second block on, the rule holds for every block. */
typedef struct ad_fx_lookahead_node {
  ad_lookahead_config config;
  int n_side, side_parents[AD_FX_MAX_PARENTS], side_ports[AD_FX_MAX_PARENTS];
} ad_fx_lookahead_node;
typedef struct ad_fx_vocoder_node {
  ad_vocoder_config config;
  int n_side, side_parents[AD_FX_MAX_PARENTS], side_ports[AD_FX_MAX_PARENTS];
} ad_fx_vocoder_node;

/* ---- crossover.MultiBand, dynamics.MultibandCompressor (dsp/filter/crossover/
 * crossover.go:113-222, dsp/effects/dynamics/multiband.go) ----------------------
 * For `channels` instances sharing one configuration.
 *
 * ad_xover: nfreq cascaded two-way Linkwitz-Riley stages, nfreq + 1 bands; the
 * highpass of a stage is the next stage's input (ProcessBlock :194-215).  Every
 * band is bit for bit the reference's: the sections run biquad.Section.
 * ProcessSample's recurrence, first-order sections included, with no FMA.
 * validate: crossover.New :32-43 and NewMultiBand :135-144 -- order positive
 *   and even, every frequency in (0, fs/2), strictly ascending -- and the
 *   kernel's limits, order <= 24 and nfreq <= 7 (maxMultibandOrder and
 *   maxMultibandBands - 1 of multiband.go:15-16).  Host only.
 * sections: host only.  The sections in use, [nfreq][2 (LP, HP)][S][5]
 *   {b0, b1, b2, a1, a2}, designed with the operations of pass.LinkwitzRileyLP /
 *   HP / HPInverted in their order, and S, the sections per side (the halved-
 *   order Butterworth prototype twice: 2, 2, 4, 4, 12 for orders 2, 4, 6, 8,
 *   24).  `sections` may be NULL to ask for S alone; cap counts doubles.
 * process: host in [channels][n], bands [nfreq + 1][channels][n].
 * process_device: band b of channel c starts at d_bands + b * band_stride +
 *   c * row_stride; in_stride, row_stride >= n, band_stride >= (channels - 1) *
 *   row_stride + n; d_in must not overlap the bands.  Calls of any length
 *   continue the stream.
 * get_state / set_state: one channel's [nfreq][2][S][2] {s0, s1}, the
 *   checkpoint surface (as ad_fx_chain_eq_state); cap and n count doubles.
 * kernel_info: waves per workgroup (one per stage in the pipelined form, 1 in
 *   the one-stage-per-launch form), samples per tile, LDS bytes of a workgroup.
 * set_pipelined: 1 (default) runs all stages in one launch as a pipeline over
 *   time tiles; 0 runs one stage per launch.  The two give the same bits.      */
typedef struct ad_xover ad_xover;
int ad_xover_validate(const double* freqs, int nfreq, int order, double sample_rate);
int ad_xover_sections(const double* freqs, int nfreq, int order, double sample_rate, double* sections, int64_t cap,
                      int* sections_per_side);
int ad_xover_create(const double* freqs, int nfreq, int order, double sample_rate, int channels, int device,
                    ad_xover** out);
int ad_xover_process(ad_xover* x, const double* in, double* bands, int64_t n);
int ad_xover_process_device(ad_xover* x, const double* d_in, int64_t in_stride, double* d_bands, int64_t row_stride,
                            int64_t band_stride, int64_t n, void* stream);
int ad_xover_get_state(ad_xover* x, int channel, double* state, int64_t cap);
int ad_xover_set_state(ad_xover* x, int channel, const double* state, int64_t n);
int ad_xover_reset(ad_xover* x);
int ad_xover_kernel_info(const ad_xover* x, int* waves_per_workgroup, int* tile, int* lds_bytes);
int ad_xover_set_pipelined(ad_xover* x, int on);
void ad_xover_destroy(ad_xover* x);

/* ad_multiband: the crossover, one dynamics.Compressor per band, the bands
 * summed in band order (ProcessInPlace :468-489).  The crossover is bit for
 * bit the reference's; each band's compressor is the ad_fx_chain compressor
 * stage with its bars.
 * validate: validateMultibandParams :661-709 -- at least one frequency, at
 *   most 8 bands, order even in [2, 24], every frequency finite, >= 20 Hz,
 *   < Nyquist, ascending.  Host only.
 * create: every band starts from ad_compressor_default_config.
 * set_band: ad_compressor_validate's rules; cfg->sample_rate must be the
 *   handle's.  A rejected config or band index changes nothing.  The band's
 *   state carries on as ad_fx_chain_set_compressor documents.
 * process / process_device: in place on [channels][n] / [channels][stride].
 * process_multi / process_multi_device: per-band outputs laid out as
 *   ad_xover_process / _process_device do; the input is not written
 *   (ProcessInPlaceMulti :507-523).
 * metrics: GetMetrics :537-544 of one band and channel; reset_metrics :547-551.
 * reset: :528-534, the crossover and every compressor.
 * xover_state: as ad_xover_get_state.
 * set_chunk: a call runs in passes of at most `samples` samples with every
 *   state carried; 0 (default): as many as keep the band planes of a pass
 *   within 2 GiB.                                                              */
typedef struct ad_multiband ad_multiband;
int ad_multiband_validate(const double* freqs, int nfreq, int order, double sample_rate);
int ad_multiband_create(const double* freqs, int nfreq, int order, double sample_rate, int channels, int device,
                        ad_multiband** out);
int ad_multiband_set_band(ad_multiband* m, int band, const ad_compressor_config* cfg);
int ad_multiband_get_band(const ad_multiband* m, int band, ad_compressor_config* cfg);
int ad_multiband_process(ad_multiband* m, double* buf, int64_t n);
int ad_multiband_process_device(ad_multiband* m, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_multiband_process_multi(ad_multiband* m, const double* in, double* bands, int64_t n);
int ad_multiband_process_multi_device(ad_multiband* m, const double* d_in, int64_t in_stride, double* d_bands,
                                      int64_t row_stride, int64_t band_stride, int64_t n, void* stream);
int ad_multiband_metrics(ad_multiband* m, int band, int channel, double* input_peak, double* output_peak,
                         double* gain_reduction);
int ad_multiband_reset_metrics(ad_multiband* m);
int ad_multiband_reset(ad_multiband* m);
int ad_multiband_xover_state(ad_multiband* m, int channel, double* state, int64_t cap);
int ad_multiband_set_chunk(ad_multiband* m, int64_t samples);
void ad_multiband_destroy(ad_multiband* m);

/* ---- effects.SpectralFreeze, pitch.SpectralPitchShifter (dsp/effects/
 * spectral_freeze.go, dsp/effects/pitch/pitch_shift_spectral.go) ---------------
 * Short-frame STFT overlap-add for `channels` instances that share one
 * configuration; buf [channels][n] (host) / [channels][stride] (device), in
 * place, one call = one Process of the whole buffer.  Frame sizes are powers of
 * two in [64, 4096]; a larger power of two, which the reference would accept,
 * is AD_ERR_INVALID_ARGUMENT (a documented limit).
 *
 * The window is a table of frame_size coefficients the caller computes
 * (window.Generate(t, N, WithPeriodic())); window_type only names it.  The
 * table is copied by create / set_frame / set_window; get_config returns NULL
 * pointers.  A stated deviation: the imaginary parts of analysis bins 0 and
 * N/2 are set to +0.0 before the polar conversion.
 *
 * ad_specfreeze: set_param follows the reference's setters (a rejected value
 * changes nothing); AD_SPECFREEZE_FROZEN clears the captured frame when the
 * value changes (SetFrozen :169-175); set_frame is SetFrameSize :115-127 with
 * the window for the new size (pulls a hop >= frame down to frame / 4, rebuilds
 * the state); set_window is SetWindowType :152-155 (rebuilds the state); reset
 * is Reset :184-189.  ad_specfreeze_state copies heldMagnitude and phaseAcc
 * [channels][frame_size / 2 + 1] and hasFrozenFrame.  ad_specfreeze_norm
 * writes the overlap-add norm of a call of n samples (host, [n]).
 *
 * ad_pitchspec: the reference's Process with its identity shortcut
 * (|ratio - 1| <= 1e-9 leaves the buffer), the bin-shift path for
 * |ratio - 1| <= 0.15 and the time stretch with resample.Resample(stretched,
 * analysisHop, synthesisHop, quality) and fitLength beyond.  The resampling
 * prototype is the caller's (designPolyphaseFIR for the reduced hops and the
 * quality's profile): resample_taps [n_resample_taps], a multiple of the
 * reduced analysis hop; a stretch call without one is AD_ERR_INVALID_ARGUMENT.
 * set_param(AD_PITCHSPEC_RATIO / HOP) and set_frame drop the prototype when
 * they change the reduced hops; ad_pitchspec_set_resample_taps installs one.  */
/* ad_*_profile(h, enable, ms): with ms, the milliseconds spent in each pass (events around the launches) by
 * the calls made since profiling was switched on, ms[AD_STFT_PASSES]; then profiling on or off. */
#define AD_STFT_PASS_ANALYSIS 0  /* window, forward transform, hypot / atan2 */
#define AD_STFT_PASS_WALK 1      /* the serial walk over frames */
#define AD_STFT_PASS_SYNTHESIS 2 /* sincos, inverse transform, window */
#define AD_STFT_PASS_OLA 3       /* overlap-add gather, norm, mix */
#define AD_STFT_PASS_RESAMPLE 4  /* the time stretch's resampling and fitLength */
#define AD_STFT_PASS_FUSED 5     /* analysis and synthesis in one kernel (the unfrozen freeze) */
#define AD_STFT_PASSES 6
typedef struct ad_specfreeze ad_specfreeze;
typedef struct ad_specfreeze_config {
  double sample_rate, mix;
  int frame_size, hop_size, phase_mode, frozen, window_type;
  const double* window; /* [frame_size] */
} ad_specfreeze_config;
#define AD_SPECFREEZE_PHASE_HOLD 0
#define AD_SPECFREEZE_PHASE_ADVANCE 1
#define AD_SPECFREEZE_SAMPLE_RATE 0 /* SetSampleRate spectral_freeze.go:104 */
#define AD_SPECFREEZE_HOP 1         /* SetHopSize :130 */
#define AD_SPECFREEZE_MIX 2         /* SetMix :141 */
#define AD_SPECFREEZE_PHASE_MODE 3  /* SetPhaseMode :158 */
#define AD_SPECFREEZE_FROZEN 4      /* SetFrozen :169 */
void ad_specfreeze_default_config(ad_specfreeze_config* cfg, double sample_rate);
int ad_specfreeze_validate(const ad_specfreeze_config* cfg);
int ad_specfreeze_create(const ad_specfreeze_config* cfg, int channels, int device, ad_specfreeze** out);
int ad_specfreeze_set_param(ad_specfreeze* f, int which, double value);
int ad_specfreeze_set_frame(ad_specfreeze* f, int frame_size, const double* window);
int ad_specfreeze_set_window(ad_specfreeze* f, int window_type, const double* window);
int ad_specfreeze_get_config(const ad_specfreeze* f, ad_specfreeze_config* cfg);
int ad_specfreeze_state(ad_specfreeze* f, double* held_magnitude, double* phase_acc, int* has_frozen);
int ad_specfreeze_norm(ad_specfreeze* f, double* norm, int64_t n);
int ad_specfreeze_process(ad_specfreeze* f, double* buf, int64_t n);
int ad_specfreeze_process_device(ad_specfreeze* f, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_specfreeze_reset(ad_specfreeze* f);
int ad_specfreeze_profile(ad_specfreeze* f, int enable, double* ms);
void ad_specfreeze_destroy(ad_specfreeze* f);

typedef struct ad_pitchspec ad_pitchspec;
typedef struct ad_pitchspec_config {
  double sample_rate, pitch_ratio;
  int frame_size, analysis_hop, window_type, resample_quality;
  const double* window;        /* [frame_size] */
  const double* resample_taps; /* [n_resample_taps], or NULL */
  int64_t n_resample_taps;
} ad_pitchspec_config;
#define AD_PITCHSPEC_SAMPLE_RATE 0      /* SetSampleRate pitch_shift_spectral.go:140 */
#define AD_PITCHSPEC_RATIO 1            /* SetPitchRatio :151 */
#define AD_PITCHSPEC_HOP 2              /* SetAnalysisHop :199 */
#define AD_PITCHSPEC_RESAMPLE_QUALITY 3 /* SetResampleQuality :217 */
void ad_pitchspec_default_config(ad_pitchspec_config* cfg, double sample_rate);
int ad_pitchspec_validate(const ad_pitchspec_config* cfg);
int ad_pitchspec_create(const ad_pitchspec_config* cfg, int channels, int device, ad_pitchspec** out);
int ad_pitchspec_set_param(ad_pitchspec* p, int which, double value);
int ad_pitchspec_set_frame(ad_pitchspec* p, int frame_size, const double* window);
int ad_pitchspec_set_window(ad_pitchspec* p, int window_type, const double* window);
int ad_pitchspec_set_resample_taps(ad_pitchspec* p, const double* taps, int64_t n_taps);
int ad_pitchspec_get_config(const ad_pitchspec* p, ad_pitchspec_config* cfg);
int ad_pitchspec_effective_ratio(const ad_pitchspec* p, double* ratio); /* EffectivePitchRatio :108-114 */
int ad_pitchspec_synthesis_hop(const ad_pitchspec* p, int* hop);        /* SynthesisHop :123-129 */
int ad_pitchspec_path(const ad_pitchspec* p, int* path);                /* 0 identity, 1 bin shift, 2 time stretch */
int ad_pitchspec_process(ad_pitchspec* p, double* buf, int64_t n);
int ad_pitchspec_process_device(ad_pitchspec* p, double* d_buf, int64_t stride, int64_t n, void* stream);
int ad_pitchspec_reset(ad_pitchspec* p);
int ad_pitchspec_profile(ad_pitchspec* p, int enable, double* ms);
void ad_pitchspec_destroy(ad_pitchspec* p);

/* ---- time-domain pitch shifter (dsp/effects/pitch/pitch_shifter.go) ----------
 * pitch.PitchShifter for `channels` channels: a WSOLA stretch (timeStretch
 * :298-357; per frame a normalised cross-correlation over 2 searchLen + 1
 * candidates, findBestOverlap :359-389) and a 4-point Hermite resample back to
 * the call's length (:391-430).  Every candidate's sums keep the reference's
 * term order, so the selections, and with them every sample, are the
 * reference's bit for bit.  The processor is stateless: a call transforms its
 * whole block, and the result depends on the length of the call as the
 * reference's does on its block.  |ratio - 1| <= 1e-9 leaves the buffer.
 *
 * It runs as the node AD_FXN_PITCHTIME of an fx graph and has no entry points
 * of its own: cfg[i] of the node is this structure with its size, through the
 * graph's cfg create call above.  The ranges are the reference's setters' and
 * rebuild's (:122-217, :252-276): ratio in [0.25, 4], sequence in [20, 120] ms,
 * overlap in [4, 60] ms and below the sequence, search in [2, 40] ms; the
 * lengths are max(round(ms * 0.001 * sample_rate), 32 / 8 / 1) with
 * overlapLen < sequenceLen and a hop of at least 4; a sample rate that makes
 * the sequence longer than 2^24 samples is refused as well.  Anything else is
 * AD_ERR_INVALID_ARGUMENT at create.  fade_in is the cross-fade's rising half,
 * [fade_len] with fade_len == overlapLen, read at create; NULL (fade_len is
 * then not read) has the library compute 0.5 - 0.5 cos(pi i / (L - 1)) with
 * its own cos.  A call takes n < 2^29 samples per channel. */
typedef struct ad_pitchtime_config {
  double sample_rate, pitch_ratio;
  double sequence_ms, overlap_ms, search_ms;
  const double* fade_in; /* [fade_len], or NULL */
  int64_t fade_len;
} ad_pitchtime_config;

/* ---- spectral correlation / deconvolution (dsp/conv/correlate.go,
 * dsp/conv/deconvolve.go) --------------------------------------
 * One power-of-two FFT over the whole zero-padded signal, as the reference's
 * algofft.NewPlan64(n) calls.  Inputs are host arrays copied in inside the
 * call (the _device form takes device pointers on a caller stream).        */

/* CorrelateFFT (correlate.go:111-172): out[n+m-1], index k = lag k-(m-1);
 * FFT size nextPow2(n+m-1); empty a or b -> AD_ERR_EMPTY_INPUT.            */
int ad_correlate_fft(const double* a, int64_t n, const double* b, int64_t m, double* out, int device);
int ad_correlate_fft_device(const double* d_a, int64_t n, const double* d_b, int64_t m, double* d_out, int device,
                            void* stream);

/* DeconvMethod / DeconvOptions (deconvolve.go:20-63) */
#define AD_DECONV_NAIVE 0
#define AD_DECONV_REGULARIZED 1
#define AD_DECONV_WIENER 2
typedef struct {
  int method;
  double epsilon;         /* Regularized: <= 0 -> 1e-6 */
  double noise_variance;  /* Wiener: <= 0 -> 1% of the signal variance */
  double signal_variance; /* Wiener: <= 0 -> variance(signal) */
} ad_deconv_options;
ad_deconv_options ad_deconv_default_options(void); /* :57-63 {Regularized, 1e-6} */

/* Deconvolve (deconvolve.go:72-101 and the three methods :104-323): circular
 * spectral division at FFT size nextPow2(n) (the signal length);
 * *out_len = n-m+1, or n when that is <= 0.  Empty signal ->
 * AD_ERR_EMPTY_INPUT, empty kernel -> AD_ERR_EMPTY_KERNEL, naive method with
 * |H[k]| < 1e-15 -> AD_ERR_DIVISION_BY_ZERO (first bin in ad_last_error);
 * m > nextPow2(n) (the reference indexes out of range) -> AD_ERR_INVALID_ARGUMENT. */
int ad_deconvolve(const double* signal, int64_t n, const double* kernel, int64_t m, const ad_deconv_options* opts,
                  double* out, int64_t out_cap, int64_t* out_len, int device);

/* InverseFilter (deconvolve.go:354-394): out[length] = real(IFFT(conj H /
 * (|H|^2 + eps))), FFT size nextPow2(length), kernel truncated to it;
 * eps <= 0 -> 1e-6; empty kernel -> AD_ERR_EMPTY_KERNEL.                   */
int ad_inverse_filter(const double* kernel, int64_t m, int64_t length, double epsilon, double* out, int device);

#ifdef __cplusplus
}
#endif

#endif /* ALGODSP_H_ */
