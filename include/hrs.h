/*
 * hrs.h — C ABI of the MI355X-native Reed-Solomon engine (libhrs.so).
 *
 * This is the drop-in boundary behind the hops codec plugin surface
 * `io.hops.erasure_coding.ErasureCode` (hadoop-hdfs-project/hadoop-hdfs/src/
 * main/java/io/hops/erasure_coding/ErasureCode.java:25-182). A JNI shim
 * (lambdafs_amd/jni/) maps the Java class
 * `io.hops.erasure_coding.HipReedSolomonCode extends ErasureCode` onto these
 * entry points exactly as the existing native precedent
 * `NativeReedSolomonCode` maps onto libhadoop's ISA-L shim
 * (hops-erasure-coding/.../NativeReedSolomonCode.java:55-152 ->
 *  hadoop-common/src/main/native/src/org/apache/hadoop/io/erasurecode/
 *  jni_rs_encoder.c:45-63, jni_rs_decoder.c:35-77).
 *
 * Semantics are those of the Java `rs` codec, `ReedSolomonCode`
 * (hops-erasure-coding/src/main/java/io/hops/erasure_coding/
 * ReedSolomonCode.java), bit-exact:
 *   - GF(2^8), primitive polynomial 0x11D, alpha = 2;
 *   - stripe locations in hops order: [0, p) parity, [p, p+k) data;
 *   - encode  = ReedSolomonCode.encodeBulk   (ReedSolomonCode.java:103-125);
 *   - decode  = ReedSolomonCode.decodeBulk 5-arg (ReedSolomonCode.java:191-211);
 *   - decode3 = ReedSolomonCode.decodeBulk 3-arg (ReedSolomonCode.java:168-185).
 *
 * Conventions: no JNI or torch types; plain pointers and sizes. Every
 * function returns HRS_OK (0) on success and a nonzero hrs_status otherwise;
 * the JNI shim turns a nonzero status into java.io.IOException
 * (HRS_ETOOMANY into io.hops.erasure_coding.TooManyErasedLocations), as
 * jni_rs_encoder.c:51 THROWs. A handle is not thread-safe (like the Java
 * ReedSolomonCode, whose scratch arrays are per instance,
 * ReedSolomonCode.java:36-38); distinct handles are fully concurrent.
 */
#ifndef HRS_H_
#define HRS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int hrs_status;
enum {
  HRS_OK = 0,
  HRS_EINVAL = 1,    /* bad argument (IllegalArgumentException / assert in Java) */
  HRS_ETOOMANY = 2,  /* ErasureCode.java:105-111 TooManyErasedLocations */
  HRS_EDEVICE = 3,   /* HIP runtime failure (no GPU, launch or copy error) */
  HRS_ENOMEM = 4,    /* device or pinned-host allocation failed */
  HRS_EALIGN = 5     /* device-batch rows not 16-byte aligned (see hrs_*_dev) */
};

typedef struct hrs_codec hrs_codec;

/* Code families behind the same boundary (hops codec table,
 * hadoop-hdfs/src/main/resources/erasure-coding-default.xml:13-56). */
enum {
  HRS_CODE_RS = 0,  /* "rs":  io.hops.erasure_coding.ReedSolomonCode (ReedSolomonCode.java) */
  HRS_CODE_XOR = 1, /* "xor": io.hops.erasure_coding.XORCode (XORCode.java), parity_size == 1 */
  HRS_CODE_SRC = 3, /* "src": io.hops.erasure_coding.SimpleRegeneratingCode (SimpleRegeneratingCode.java):
                     * RS(k, r) plus s local XOR parities; create with hrs_create_src.
                     * Locations [SRC parities 0..s-1, RS parities s..p-1, data p..k+p-1].
                     * Variable-length locationsToReadForDecode (hrs_locations_to_read_list);
                     * a one-erasure decode XORs the locations to read (device calls: every
                     * location outside not_to_read); no 3-arg decode. */
  HRS_CODE_NRS = 2  /* "nrs": io.hops.erasure_coding.NativeReedSolomonCode (NativeReedSolomonCode.java)
                     * over libhadoop's ISA-L shim (erasure_coder.c): Cauchy RS, Apache
                     * [data, parity] coding order behind the hops [parity, data] locations.
                     * Decode outputs follow the Java's ordering: output t is the t-th
                     * not-to-read location in Apache order (needs num_erased <= num_not_to_read
                     * <= parity_size). No 3-arg decode (hrs_decode3 -> HRS_EINVAL). The
                     * reference's native limits (k <= 10, k + p <= 14) are lifted. */
};

#define HRS_DEVICE_NONE (-2)

typedef struct hrs_opts {
  int device;         /* HIP device ordinal; -1 = current device; HRS_DEVICE_NONE =
                         host-only handle (matrix/location queries; coding calls
                         fail with HRS_EDEVICE) */
  int reserved[7];    /* must be zero */
} hrs_opts;

/* ---- lifecycle (ReedSolomonCode() + init(Codec), ReedSolomonCode.java:45-82) ---- */

/* Builds the generator polynomial and encode matrix for RS(stripe_size,
 * parity_size). Requires stripe_size >= 1, parity_size >= 1 and
 * stripe_size + parity_size < 256 (ReedSolomonCode.java:57). opts may be NULL. */
hrs_status hrs_create(int stripe_size, int parity_size, const hrs_opts* opts, hrs_codec** out);
/* Same for any code family: HRS_CODE_RS (== hrs_create), HRS_CODE_XOR
 * (XORCode.init asserts parity_size == 1, XORCode.java:46-51) or HRS_CODE_NRS
 * (NativeReedSolomonCode.init, NativeReedSolomonCode.java:44-51). */
hrs_status hrs_create_code(int code, int stripe_size, int parity_size, const hrs_opts* opts,
                           hrs_codec** out);
int hrs_code_kind(const hrs_codec* codec);
/* SimpleRegeneratingCode.init(Codec) (SimpleRegeneratingCode.java:52-114):
 * src_parity_size = the codec's "parity_length_src" (the adjustment loop of
 * init may lower it; hrs_src_layout reports what it settled on). */
hrs_status hrs_create_src(int stripe_size, int parity_size, int src_parity_size, const hrs_opts* opts,
                          hrs_codec** out);
/* SRC layout after init: stored SRC parities s, RS parities r = p - s, and
 * the group degree d (locations per stored SRC group). */
hrs_status hrs_src_layout(const hrs_codec* codec, int* src_parities, int* rs_parities, int* group_degree);
void hrs_destroy(hrs_codec* codec);
/* Last error message of this handle ("" if none); handle may be NULL for create errors. */
const char* hrs_last_error(const hrs_codec* codec);
/* Name of the main kernel the handle's latest coding call launched, as
 * rocprofv3 prints it without its namespace and parameters (e.g.
 * "encode_static_kernel<10, 4>"); "" before any device work. A call that
 * launches a vector kernel and a byte-granular kernel for the row tails names
 * the vector kernel (with several vector launches, the last one); a call whose
 * only launch is the byte-granular kernel (rows or strides off 16-byte
 * boundaries, rows shorter than 2 KiB, kernel mode 2) names that one
 * ("bytewise_kernel", "batch_bytewise_kernel"); a call that launches no kernel
 * (hrs_apply_dev with an all-zero matrix) sets "". hrs_crc32_dev leaves the
 * name alone. Lets a benchmark attach the PMC traffic of the kernel it
 * actually ran. */
const char* hrs_last_kernel(const hrs_codec* codec);
/* How the handle's latest synchronous host-buffer call (hrs_encode, hrs_decode,
 * hrs_decode3, hrs_*_crc) or host batch (hrs_*_batch_host) moved its bytes:
 * "pinned" (rows or batch in memory the runtime allocated pinned —
 * hipHostMalloc, torch pin_memory —: the zero-copy kernel in place),
 * "staged" (any other host memory, pageable or registered by the caller with
 * hipHostRegister, copied through the library's pinned staging, the zero-copy
 * kernel on the staging; the default), "copy_engine" (staging, H2D, kernel,
 * D2H), or "" before any such call. The GPU never reads or writes
 * caller-registered pageable memory in place: registration does not pin its
 * pages ("Platform constraint"). Diagnostic, like
 * hrs_last_kernel. */
const char* hrs_last_host_path(const hrs_codec* codec);
const char* hrs_version(void);

/* ---- device set (SURVEY §5 "engine env/config for device set"; §8(e)) ----
 * The reference creates one codec per Encoder / Decoder through
 * Codec.createErasureCode -> ReflectionUtils.newInstance(class, conf) -> init
 * (hadoop-hdfs/.../io/hops/erasure_coding/Codec.java:200-213). A binding picks
 * the GPU of each handle with hrs_opts.device (the Java classes: round robin
 * over the conf key hdfs.raid.hip.devices). */

/* HIP devices visible to this process (HIP_VISIBLE_DEVICES applies); 0 if the
 * HIP runtime finds none. Valid ordinals for hrs_opts.device are [0, count). */
int hrs_device_count(void);
/* Device ordinal a handle runs on (HRS_DEVICE_NONE for a host-only handle,
 * -1 for NULL). */
int hrs_codec_device(const hrs_codec* codec);

/* ErasureCode.stripeSize()/paritySize()/symbolSize() (ReedSolomonCode.java:213-226). */
int hrs_stripe_size(const hrs_codec* codec);
int hrs_parity_size(const hrs_codec* codec);
int hrs_symbol_size(const hrs_codec* codec);

/* ---- host helpers (no device work) ---- */

/* locationsToReadForDecode as a list of variable length, for every code
 * family (SRC returns a local group; the others exactly stripe_size
 * locations, as hrs_locations_to_read): to_read has room for k + p entries,
 * *num_to_read receives the count. SimpleRegeneratingCode.java:300-366,
 * ErasureCode.java:89-113. */
hrs_status hrs_locations_to_read_list(const hrs_codec* codec, const int* erased, int num_erased, int* to_read,
                                      int* num_to_read);

/* ErasureCode.locationsToReadForDecode (ErasureCode.java:89-113): writes the
 * k = stripe_size highest-index locations not in `erased` to to_read, in
 * descending order, as the Java list is built. HRS_ETOOMANY if fewer than k
 * survive. */
hrs_status hrs_locations_to_read(const hrs_codec* codec, const int* erased, int num_erased,
                                 int* to_read);

/* p x k encode matrix G (row-major): parity_r = XOR_c G[r][c] * data_c.
 * XOR code: one row of ones (XORCode.encodeBulk, XORCode.java:99-113). */
hrs_status hrs_encode_matrix(const hrs_codec* codec, uint8_t* g);

/* num_erased x n decode matrix D (row-major, n = k + p, hops order):
 * out_i = XOR_l D[i][l] * in_l.
 * zero_not_to_read = 1: decodeBulk 5-arg semantics (ReedSolomonCode.java:144-166,
 *   191-211): locations in not_to_read are zeroed, m = num_not_to_read
 *   syndromes, erased locations absent from not_to_read decode to 0.
 * zero_not_to_read = 0: decodeBulk 3-arg semantics (ReedSolomonCode.java:168-185):
 *   not_to_read is the erased list itself, nothing is zeroed.
 * RS: D is the reference decode run on unit vectors, so it reproduces the
 * Java on every list the Java accepts: repeated locations (a division by zero
 * in solveVandermondeSystem yields 0, GaloisField.java:107-118) and, in the
 * 5-arg form, erased locations of any value (only compared with not_to_read).
 * not_to_read locations (and 3-arg erased ones) must be in [0, n). */
hrs_status hrs_decode_matrix(const hrs_codec* codec, const int* erased, int num_erased,
                             const int* not_to_read, int num_not_to_read, int zero_not_to_read,
                             uint8_t* d);

/* ---- synchronous host-buffer calls: the JNI path (GetPrimitiveArrayCritical rows) ---- */

/* ReedSolomonCode.encodeBulk(byte[][] inputs, byte[][] outputs):
 * inputs[k] rows and outputs[p] rows, each `len` bytes, host memory.
 * Outputs are fully overwritten. Unlike the Java method (whose bulk
 * remainder zeroes `inputs`, GaloisField.java:326-338) inputs are left
 * untouched; the Java/Python shims restore that side effect when asked. */
hrs_status hrs_encode(hrs_codec* codec, const uint8_t* const* inputs, uint8_t* const* outputs,
                      size_t len);

/* XOR code: decode needs exactly one erased location; the output is the XOR
 * of every other row (XORCode.decodeBulk, XORCode.java:115-145; NULL rows
 * count as the zeros the reference reads there). */

/* ReedSolomonCode.decodeBulk(readBufs, writeBufs, erased, toRead, notToRead)
 * (ReedSolomonCode.java:191-211): read_bufs[n] in hops order (a row may be
 * NULL when its location is in not_to_read — the reference feeds zeros
 * there, StripeReader.java:111-120); write_bufs[num_erased], row i = value at
 * erased[i]. to_read is accepted for interface parity; like the Java code the
 * result depends only on erased and not_to_read. */
hrs_status hrs_decode(hrs_codec* codec, const uint8_t* const* read_bufs, uint8_t* const* write_bufs,
                      const int* erased, int num_erased, const int* to_read, int num_to_read,
                      const int* not_to_read, int num_not_to_read, size_t len);

/* ReedSolomonCode.decodeBulk(readBufs, writeBufs, erasedLocation)
 * (ReedSolomonCode.java:168-185): all n rows are read as given. */
hrs_status hrs_decode3(hrs_codec* codec, const uint8_t* const* read_bufs, uint8_t* const* write_bufs,
                       const int* erased, int num_erased, size_t len);

/* hrs_encode plus the block checksums Encoder.encodeStripe keeps when
 * computeBlockChecksum is set (Encoder.java:408-450: sourceChecksums[i].update
 * over readBufs[i], parityChecksums[i].update over writeBufs[i]):
 * crc_out[r] = java.util.zip.CRC32 continued from crc_in[r] over input row r
 * (r < k) or output row r - k (r >= k). crc_in / crc_out are HOST arrays of
 * k + p uint32 (crc_in NULL = fresh CRC32 objects; crc_out may alias crc_in).
 * Each cell is checksummed on the GPU as it passes through, in the same
 * pipelined copy as the encode; no second host pass. */
hrs_status hrs_encode_crc(hrs_codec* codec, const uint8_t* const* inputs, uint8_t* const* outputs,
                          size_t len, const uint32_t* crc_in, uint32_t* crc_out);

/* hrs_decode plus the CRC-32 of every repaired row (Decoder.java:222-229 and
 * :645-655 compare it with the block checksum the NameNode holds):
 * crc_out[i] = CRC32 continued from crc_in[i] over write_bufs[i]. HOST arrays
 * of num_erased uint32 (crc_in NULL = fresh). */
hrs_status hrs_decode_crc(hrs_codec* codec, const uint8_t* const* read_bufs, uint8_t* const* write_bufs,
                          const int* erased, int num_erased, const int* to_read, int num_to_read,
                          const int* not_to_read, int num_not_to_read, size_t len,
                          const uint32_t* crc_in, uint32_t* crc_out);

/* ---- asynchronous host-buffer calls: successive rounds overlap ----
 * An Encoder / Decoder round (Encoder.java:421-453, Decoder.java:280-372)
 * split in two. *_submit copies the caller's rows into a free slot's pinned
 * staging — the rows may be reused or freed as soon as it returns (the JNI
 * shim pins Java arrays only for the call) — queues H2D -> kernel -> D2H on
 * the slot's stream and returns a ticket; hrs_collect waits for that
 * operation and copies its output rows out. While round r runs on the GPU the
 * caller reads round r + 1 and submits it. A handle holds up to 4 uncollected
 * operations (more -> HRS_EINVAL); tickets may be collected in any order.
 * checksums = 1 adds the block CRC-32s of hrs_encode_crc / hrs_decode_crc:
 * the running values are chained at collect time (rounds are collected in
 * order), so they need not be known when the round is submitted. */
hrs_status hrs_encode_submit(hrs_codec* codec, const uint8_t* const* inputs, size_t len, int checksums,
                             uint64_t* ticket);
hrs_status hrs_decode_submit(hrs_codec* codec, const uint8_t* const* read_bufs, const int* erased,
                             int num_erased, const int* to_read, int num_to_read, const int* not_to_read,
                             int num_not_to_read, size_t len, int checksums, uint64_t* ticket);
/* outputs: p rows (encode) or num_erased rows (decode) of `len` bytes.
 * crc_io (checksummed operations only): k + p (sources, then parities) or
 * num_erased running java.util.zip.CRC32 values (0 = a fresh CRC32), each
 * continued over this operation's cell (CRC32.update chaining). */
hrs_status hrs_collect(hrs_codec* codec, uint64_t ticket, uint8_t* const* outputs, uint32_t* crc_io);
/* Waits until the operation's H2D, kernel and D2H have completed, without
 * copying anything out or releasing it (hrs_collect still must be called;
 * it then returns without blocking). Lets a binding wait before it pins the
 * caller's output rows: the JNI shim calls it outside any
 * GetPrimitiveArrayCritical region. HRS_EINVAL for an unknown ticket. */
hrs_status hrs_wait(hrs_codec* codec, uint64_t ticket);
/* Drops an uncollected operation without copying anything out: its slot's
 * stream is drained (whatever state its GPU work ended in) and the slot
 * freed for the next submit. For a binding that gives up on a round — the
 * JNI shim calls it when hrs_wait fails, before the IOException reaches
 * Java, so a caller that treats the exception as final does not lose one of
 * the handle's 4 slots. HRS_EINVAL for an unknown ticket; the drain's HIP
 * error if it fails (the slot is freed either way). */
hrs_status hrs_release(hrs_codec* codec, uint64_t ticket);
/* Uncollected operations of this handle. */
int hrs_pending(const hrs_codec* codec);
/* Diagnostic: with timing on (hrs_set_timing(codec, 1); off by default), each
 * submitted operation records a timing event before its first GPU operation
 * and one after its last, on its slot's stream; hrs_ticket_gpu_ms then gives
 * the GPU-side launch-to-completion time of a waited-for (hrs_wait) and not
 * yet collected operation. HRS_EINVAL for an unknown ticket or an operation
 * submitted with timing off. Lets a benchmark put the GPU time of small
 * asynchronous rounds beside their wall time. */
hrs_status hrs_set_timing(hrs_codec* codec, int on);
hrs_status hrs_ticket_gpu_ms(const hrs_codec* codec, uint64_t ticket, float* ms);
/* Shape of an uncollected operation: output rows, their length, CRC values
 * (0 if not checksummed). HRS_EINVAL for an unknown ticket. */
hrs_status hrs_ticket_shape(const hrs_codec* codec, uint64_t ticket, int* num_outputs, size_t* len, int* num_crcs);

/* ---- device-resident batches (the MI355X hot path) ----
 * Row pointers are DEVICE pointers for stripe 0; stripe s of row r lives at
 * rows[r] + s * stride. `stream` is a hipStream_t (NULL = the null stream).
 * Calls are asynchronous on `stream`. For the vector path every row pointer
 * and stride must be 16-byte aligned; otherwise a byte-granular kernel runs. */

/* Encode nstripes stripes: in_rows[k] data rows -> out_rows[p] parity rows. */
hrs_status hrs_encode_dev(hrs_codec* codec, const uint8_t* const* in_rows, size_t in_stride,
                          uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                          void* stream);

/* decodeBulk 5-arg over nstripes stripes: rows[n] in hops order (entries for
 * not_to_read locations may be NULL), out_rows[num_erased]. */
hrs_status hrs_decode_dev(hrs_codec* codec, const uint8_t* const* rows, size_t in_stride,
                          uint8_t* const* out_rows, size_t out_stride, const int* erased,
                          int num_erased, const int* not_to_read, int num_not_to_read, size_t len,
                          size_t nstripes, void* stream);

/* Repair of a batch whose stripes lost different locations (a repair job over
 * many stripes: Decoder.fixErasedBlockImpl / recoverBlock per stripe,
 * Decoder.java:291-338), in one launch. Stripe s holds location l at
 * stripes + s * stripe_stride + l * row_stride (hops order). Its erased
 * locations are erased[s * max_erased + t] for t < max_erased up to the first
 * negative entry (zero erasures allowed). Each stripe is decoded like
 * hrs_decode_dev with the survivors locationsToReadForDecode picks and every
 * other location not read (Decoder.java:303-338); output t of stripe s goes to
 * out + s * out_stripe_stride + t * out_row_stride. HRS_ETOOMANY if a stripe
 * lost more than the code repairs. */
hrs_status hrs_decode_batch_dev(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                size_t nstripes, void* stream);

/* ---- host-memory batches: many stripes per call, pipelined ----
 * Stripes start and end in host memory (DataNode sockets / local block files;
 * Encoder.encodeFile over a file's stripes, Encoder.java:289-382; a repair job
 * over many stripes, BlockReconstructor -> Decoder.fixErasedBlockImpl per
 * stripe, Decoder.java:232-401). The stripes flow in chunks through a ring of
 * device slots, each on its own stream: H2D of exactly the rows the chunk's
 * code reads, the kernel, D2H of exactly the rows it writes, successive chunks
 * overlapping. Buffers the runtime allocated pinned (hipHostMalloc, torch
 * pin_memory) are used in place (zero copy; or DMA'd directly with
 * HRS_ZEROCOPY=0) and the whole job is queued at once; any other buffer —
 * pageable, or pageable memory the caller registered with hipHostRegister,
 * whose pages are not pinned — is staged through the handle's pinned slots by
 * the copy pool. Synchronous: outputs are in place when the call returns.
 * Rows need no alignment. */

/* hrs_decode_batch_dev over host memory (same layout, semantics and errors):
 * stripe s holds location l at stripes + s * stripe_stride + l * row_stride;
 * only the survivors each stripe's pattern reads cross PCIe (k of the n for
 * rs; fewer for src local groups), and output t of stripe s lands at
 * out + s * out_stripe_stride + t * out_row_stride. */
hrs_status hrs_decode_batch_host(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                 size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                 size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                 size_t nstripes);

/* encodeBulk of every stripe of a host batch, in place: reads data rows
 * (hops locations p..n-1) and writes parity rows (locations 0..p-1) of stripe
 * s at stripes + s * stripe_stride + l * row_stride. Only the k data rows go
 * H2D and the p parity rows D2H. */
hrs_status hrs_encode_batch_host(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                 size_t len, size_t nstripes);

/* The two host batches above over a device set: codecs[0..ncodecs) are
 * distinct handles of one code (same family, stripe and parity size; SRC:
 * same layout), each created on the device it should use (hrs_opts.device;
 * a device may appear more than once). The stripes are split into ncodecs
 * contiguous ranges of equal size (+-1 stripe), range i = stripes
 * [i * nstripes / ncodecs, (i + 1) * nstripes / ncodecs), and range i runs as
 * one hrs_*_batch_host call of codecs[i] on its own host thread (range 0 on
 * the caller's), so every device moves its own share over its own host link
 * (contiguous stripe ranges, one host thread and stream per
 * device, no data exchange between devices). Same layout, semantics and
 * results as the single-handle call; synchronous. On failure the first
 * failing range's status is returned and its message is recorded on
 * codecs[0] (hrs_last_error(codecs[0]); hrs_last_error(NULL) for a set
 * rejected before any range ran with a NULL codecs array). The handles must
 * not be used by other threads during the call. */
hrs_status hrs_decode_batch_host_multi(hrs_codec* const* codecs, int ncodecs, const uint8_t* stripes,
                                       size_t row_stride, size_t stripe_stride, const int* erased, int max_erased,
                                       uint8_t* out, size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                       size_t nstripes);
hrs_status hrs_encode_batch_host_multi(hrs_codec* const* codecs, int ncodecs, uint8_t* stripes, size_t row_stride,
                                       size_t stripe_stride, size_t len, size_t nstripes);

/* Generic GF(2^8) matrix x rows: out_o = XOR_i m[o * nin + i] * in_i (m on
 * the host, row-major nout x nin). Used with coding matrices broadcast over
 * RCCL, and by the 3-arg decode. nin, nout in [1, 255]. */
hrs_status hrs_apply_dev(hrs_codec* codec, const uint8_t* m, int nout, int nin,
                         const uint8_t* const* in_rows, size_t in_stride, uint8_t* const* out_rows,
                         size_t out_stride, size_t len, size_t nstripes, void* stream);

/* CRC-32 of device-resident cells, as java.util.zip.CRC32 (zlib) computes it
 * for the block checksums the hops drivers keep (Encoder.java:408-450,
 * Decoder.java:222-229): crc_out[s * nrows + r] = CRC32 of `len` bytes at
 * rows[r] + s * stride, continuing from crc_in[s * nrows + r] (CRC32.update
 * chaining across cells; crc_in NULL = a fresh CRC32). crc_in / crc_out are
 * DEVICE arrays of nstripes * nrows uint32. Asynchronous on `stream`. */
hrs_status hrs_crc32_dev(hrs_codec* codec, const uint8_t* const* rows, int nrows, size_t stride, size_t len,
                         size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* Encode + CRC-32 in one pass (Encoder.encodeStripe with computeBlockChecksum:
 * sourceChecksums over the read buffers, then encodeBulk, then parityChecksums
 * over the write buffers; Encoder.java:408-450). Same rows as hrs_encode_dev;
 * crc_out[s * (k + p) + r] = CRC32 of data row r (r < k) or of parity row r - k
 * (r >= k) of stripe s, continuing from crc_in (same layout; NULL = fresh).
 * rs / nrs codes with a compile-time kernel ((10,4), (6,3), (3,2), (12,4) rs;
 * (10,4), (6,3) nrs), len a multiple of 2 KiB and 16-byte-aligned rows take
 * one fused kernel (each cell read once); anything else runs hrs_encode_dev
 * then the CRC pass, with identical results. Asynchronous on `stream`. */
hrs_status hrs_encode_crc_dev(hrs_codec* codec, const uint8_t* const* in_rows, size_t in_stride,
                              uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                              const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* Repair + CRC-32 of the repaired cells in one pass (Decoder: decodeBulk, then
 * the repaired block's CRC32 compared with the NameNode's checksum;
 * Decoder.java:222-229, :352-353, :645-655). Same rows and semantics as
 * hrs_decode_dev; crc_out[s * num_erased + t] = CRC32 of output t of stripe
 * s, continuing from crc_in (same layout; NULL = fresh). DEVICE crc arrays.
 * Repairs of <= 4 locations from <= 12 live survivors (<= 8 at 4 outputs),
 * len a multiple of 2 KiB and 16-byte-aligned rows take one fused kernel
 * (each repaired cell written once, never read back); anything else runs
 * hrs_decode_dev then the CRC pass, with identical results. Asynchronous on
 * `stream`. */
hrs_status hrs_decode_crc_dev(hrs_codec* codec, const uint8_t* const* rows, size_t in_stride,
                              uint8_t* const* out_rows, size_t out_stride, const int* erased, int num_erased,
                              const int* not_to_read, int num_not_to_read, size_t len, size_t nstripes,
                              const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* ---- batches + CRC-32: the block checksums of the many-stripe calls ----
 * Encoder.encodeStripe checksums every source and parity cell
 * (Encoder.java:408-450) and the Decoder compares every repaired block's CRC32
 * with the NameNode's (Decoder.java:222-229, :645-655); these are the batch
 * calls above with those CRCs computed in the same pass. Common rules:
 *  - the bytes written to `out` / the stripes are exactly those of the call
 *    without CRCs: same layout, survivor choice, HRS_ETOOMANY, bytes left
 *    untouched, for every code family;
 *  - crc_out[i] is the zlib CRC-32 of cell i continued from crc_in[i]
 *    (CRC32.update chaining; crc_in NULL = a fresh CRC32);
 *  - crc_out may be the same array as crc_in; any other overlap of the two is
 *    HRS_EINVAL; a NULL crc_out with work to do is HRS_EINVAL;
 *  - len == 0 or nstripes == 0 (decode: or max_erased == 0) returns HRS_OK
 *    and touches nothing, the CRC arrays included;
 *  - argument errors are reported before the device is selected; a host-only
 *    handle with valid arguments gets HRS_EDEVICE;
 *  - hrs_last_kernel and hrs_last_host_path behave as for the sibling call. */

/* hrs_decode_batch_dev + the CRC-32 of every repaired cell.
 * crc_in / crc_out: DEVICE uint32 [nstripes * max_erased];
 * crc_out[s * max_erased + t] belongs to output t of stripe s. For t >= the
 * stripe's number of losses (a stripe that lost nothing included) the CRC is
 * continued over no bytes: crc_out = crc_in, or 0 when crc_in is NULL.
 * Batches of <= 4 losses per stripe from <= 12 live survivors (<= 8 at 4
 * losses), len a multiple of 2 KiB, base pointers and the four strides
 * 16-byte aligned take one fused kernel (each repaired cell written once,
 * never read back); anything else runs hrs_decode_batch_dev, then the CRC pass
 * over `out` (which reads, and discards, the rows past a stripe's losses),
 * with identical results. Asynchronous on `stream`. */
hrs_status hrs_decode_batch_crc_dev(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                    size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                    size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                    size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* hrs_decode_batch_host + the same CRCs, computed on the GPU as the chunks
 * pass through it; crc_in / crc_out are HOST uint32 [nstripes * max_erased]
 * (read before the first chunk, written once after the last). Synchronous. */
hrs_status hrs_decode_batch_host_crc(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                     size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                     size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                     size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out);

/* hrs_encode_batch_host + the CRC-32 of all k + p cells of every stripe;
 * crc_in / crc_out are HOST uint32 [nstripes * (k + p)], ordered as
 * hrs_encode_crc_dev: crc_out[s * (k + p) + r] is data row r (hops location
 * p + r) for r < k and parity row r - k for r >= k. The shapes
 * hrs_encode_crc_dev fuses take its one-pass kernel per chunk. Synchronous. */
hrs_status hrs_encode_batch_host_crc(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                     size_t len, size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out);

/* ---- ragged encode: per-cell valid lengths, zero tails never read ----
 * Every file ends in a stripe that is not full. Where the reference has no
 * source bytes for a cell it feeds zeros and reads nothing: a ZeroInputStream
 * for every block past the end of the file (FileStripeReader.java:56-67,
 * :96-104; StripeReader.java:111-120), and RaidUtils.readTillEnd zero-fills
 * the rest of a buffer at EOF and returns the bytes it really read
 * (RaidUtils.java:45-80), which ParallelStreamReader.ReadResult.numRead carries
 * per stream (ParallelStreamReader.java:54-64, :236-249) to
 * Encoder.encodeStripe (Encoder.java:437-442). A ragged batch is an ordinary
 * encode batch plus that count:
 *   - valid is a HOST array of uint32_t[nstripes * k];
 *   - valid[s * k + j] is the number of leading bytes of data cell j of stripe
 *     s (hops location p + j) that hold data;
 *   - the cell is taken to be those bytes followed by len - valid zeros,
 *     exactly the buffer readTillEnd hands encodeBulk.
 * The calls guarantee:
 *   - parity is bit-exact with encodeBulk over the zero-filled cells, for every
 *     code family a handle can have (rs, nrs, xor, src);
 *   - bytes of a cell at or beyond valid never influence any output, whatever
 *     they hold;
 *   - the storage of the whole cell (len bytes) must still be addressable;
 *   - the vector kernel loads no 2 KiB window that lies wholly at or beyond
 *     valid; the one window that contains the boundary is loaded and masked;
 *   - the staged host path copies in no byte at or beyond valid;
 *   - data cells are never written; parity rows are fully written.
 * Argument rules, in this order: a NULL handle is HRS_EINVAL with no message;
 * a NULL pointer argument, valid included, is HRS_EINVAL (a caller with full
 * stripes uses the plain call); len == 0 or nstripes == 0 returns HRS_OK and
 * touches nothing; len > UINT32_MAX or a valid entry > len is HRS_EINVAL with
 * the stripe and row named, and so is a NULL row pointer; only then the device
 * is selected (HRS_EDEVICE for a host-only handle). Argument errors come
 * before any byte is copied.
 * Kernels: rs (3,2), (6,3), (10,4), (12,4) and nrs (10,4), (6,3) with 16-byte
 * aligned rows and strides take encode_ragged_kernel<K, P> over the whole
 * 2 KiB windows; the row tail, unaligned layouts, kernel mode 2 and every
 * other code or shape take encode_ragged_bytewise_kernel (hrs_last_kernel
 * names them by the plain encode's tail rule). A batch whose every entry
 * equals len runs the plain encode itself and hrs_last_kernel names that
 * kernel, so always calling the ragged form costs nothing (kernel modes 2 and
 * 3 keep the ragged kernels even then; hrs_set_kernel_mode).
 * Not covered, by design: the synchronous single-stripe host call, the JNI
 * overloads (of the CRC forms below too). Ragged survivors in the repair
 * calls: "ragged repair" below; ragged cells at rest: "ragged scrub and heal". */

/* hrs_encode_dev's rows and layout plus valid. Asynchronous on stream; valid
 * is copied before the call returns (through the handle's per-call table
 * slots) and may be reused at once. */
hrs_status hrs_encode_ragged_dev(hrs_codec* codec, const uint8_t* const* in_rows, size_t in_stride,
                                 uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                                 const uint32_t* valid, void* stream);

/* hrs_encode_batch_host's layout plus valid, in place. Runtime-pinned stripes
 * run as one zero-copy launch: dead windows never cross the host link. Any
 * other memory is staged through the host-batch pipeline with only the valid
 * bytes of each data cell copied in (and, with HRS_ZEROCOPY=0, sent to the
 * device). hrs_last_host_path as for hrs_encode_batch_host, set only on
 * success. Synchronous. */
hrs_status hrs_encode_ragged_batch_host(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                        size_t len, size_t nstripes, const uint32_t* valid);

/* ---- ragged encode + CRC-32: the block checksums of a file's last stripe ----
 * Encoder.encodeStripe with computeBlockChecksum checksums every source buffer
 * over its FULL length, zero fill included (updateChecksums:
 * checksums[i].update(buffs[i], 0, buffs[0].length)), and every parity buffer
 * (Encoder.java:408-460). These are the two ragged calls above with those
 * CRCs from the same pass; their semantics are the product of the ragged
 * contract and the "batches + CRC-32" rules, nothing new is defined:
 *   - parity and every untouched byte are exactly what the ragged sibling
 *     leaves; valid is a HOST uint32_t[nstripes * k] array, free on return;
 *     bytes at or beyond valid never influence any output, a CRC included;
 *     data cells are never written;
 *   - the CRC layout is hrs_encode_crc_dev's: crc_out[s * (k + p) + r] is data
 *     row r for r < k and parity row r - k otherwise, continued from crc_in
 *     (NULL = fresh); a data row's value is the zlib CRC-32 of its valid bytes
 *     followed by len - valid zeros, the buffer readTillEnd hands
 *     updateChecksums;
 *   - crc_out may be crc_in itself; any other overlap is HRS_EINVAL.
 * Argument rules, in this order: a NULL handle is HRS_EINVAL with no message;
 * a NULL pointer argument (valid, crc_out, the row arrays, the stripes) is
 * HRS_EINVAL; len == 0 or nstripes == 0 returns HRS_OK and touches nothing,
 * the CRC arrays included; len > UINT32_MAX, a valid entry > len (the stripe
 * and row named) or a NULL row pointer is HRS_EINVAL; then the overlap rule of
 * the CRC arrays; only then the device is selected (HRS_EDEVICE for a
 * host-only handle). Argument errors come before any byte is copied.
 * Kernels: the shapes hrs_encode_crc_dev fuses (rs (3,2), (6,3), (10,4),
 * (12,4) and nrs (10,4), (6,3), len a multiple of 2 KiB, 16-byte aligned rows
 * and strides, kernel mode 0 or 3) take encode_ragged_crc_kernel: a dead 2 KiB
 * sub-window of a data row costs no load and no table lookup, the one that
 * holds the boundary is masked before the CRC sees it. Anything else runs the
 * ragged encode, then crc_ragged_window_kernel over the k + p rows (which
 * loads no byte at or beyond valid) and the fold, with identical results;
 * hrs_last_kernel then names the ragged encode's kernel. A batch whose every
 * entry equals len runs hrs_encode_crc_dev's route in kernel modes 0 and 1 and
 * hrs_last_kernel names that kernel, so always calling this form costs the
 * scan of valid; mode 3 keeps the ragged fused kernel for its shapes even
 * then, mode 2 forces the byte-granular route, modes 1 and 2 never fuse.
 * HRS_RAGGED_CRC_SUBS = 1 | 2 | 4 | 8 | 16 (read per call; ignored when len is
 * not a multiple of that many 2 KiB sub-windows) overrides the fused kernel's
 * window size, for tests and A/B runs.
 * Not covered, by design: the synchronous single-stripe host call, the JNI
 * overload. Ragged survivors in the repair calls: "ragged repair" below; the
 * repaired cells' CRCs, which cover no zero fill: "ragged repair + CRC-32";
 * ragged cells at rest: "ragged scrub and heal". */

/* hrs_encode_ragged_dev + the CRC-32 of all k + p cells of every stripe.
 * crc_in / crc_out: DEVICE uint32 [nstripes * (k + p)]. Asynchronous on
 * stream; valid is copied before the call returns. */
hrs_status hrs_encode_ragged_crc_dev(hrs_codec* codec, const uint8_t* const* in_rows, size_t in_stride,
                                     uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                                     const uint32_t* valid, const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* hrs_encode_ragged_batch_host + the same CRCs; crc_in / crc_out are HOST
 * uint32 [nstripes * (k + p)] (read before the first chunk, written once after
 * the last). Runtime-pinned stripes run as one zero-copy launch in place: dead
 * windows never cross the host link. hrs_last_host_path as for the sibling,
 * set only on success. Synchronous. */
hrs_status hrs_encode_ragged_batch_host_crc(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                            size_t len, size_t nstripes, const uint32_t* valid,
                                            const uint32_t* crc_in, uint32_t* crc_out);

/* ---- ragged repair: per-cell lengths, zero tails never read or written ----
 * locationsToReadForDecode picks the k highest-index live locations, in hops
 * order [parity..., data...] the data cells at the end of the stripe: the
 * cells a file tail leaves empty. The reference reads none of them: survivors
 * past the end of the file are ZeroInputStreams (StripeReader.java:111-120),
 * RaidUtils.readTillEnd zero-fills a short read, ParallelStreamReader.
 * ReadResult.numRead carries the real count (ParallelStreamReader.java:236-249)
 * to Decoder.java:349-358, and the repaired block is written and checksummed
 * only up to toWrite = min(bufSize, limit - written), limit being the lost
 * block's real length (Decoder.java:345-346, :360-369). A ragged repair batch
 * is hrs_decode_batch_dev / hrs_decode_batch_host (layout, erased, survivor
 * choice, HRS_ETOOMANY and the code families rs, nrs, xor, src exactly theirs)
 * plus one number per cell:
 *   - valid is a HOST array of uint32_t[nstripes * n] in hops order;
 *   - valid[s * n + l] is the length of cell l of stripe s.
 * The calls guarantee:
 *   - a survivor the stripe's plan reads counts as its valid leading bytes
 *     followed by len - valid zeros; bytes at or beyond valid never influence
 *     an output, whatever they hold; the storage of the whole cell (len bytes)
 *     must still be addressable;
 *   - output t of stripe s, rebuilding location e = erased[s * max_erased + t],
 *     receives exactly its first valid[s * n + e] bytes, bit-exact with
 *     decodeBulk (5-arg, as the sibling runs it) over the zero-filled
 *     survivors; bytes of the output at or beyond that length are not written
 *     and keep what they held; outputs are never read;
 *   - entries of locations a stripe neither reads nor lost are ignored, but
 *     still range-checked;
 *   - the vector kernel loads no 2 KiB window of a survivor that lies wholly
 *     at or beyond its valid, loads and masks the one window that holds the
 *     boundary, and loads nothing at all for a window in which every output of
 *     the stripe is dead;
 *   - the staged host path copies in no survivor byte at or beyond valid and
 *     copies back no output byte at or beyond it (with HRS_ZEROCOPY=0 no such
 *     byte is sent to or fetched from the device); runtime-pinned batches run
 *     as one zero-copy launch in place;
 *   - stripes that lost nothing write nothing; hrs_last_host_path behaves as
 *     for the sibling and is set only on success.
 * Argument rules, in this order: a NULL handle is HRS_EINVAL with no message;
 * the sibling's argument block (stripes, out, max_erased, erased); a NULL valid
 * is HRS_EINVAL; len == 0, nstripes == 0 or max_erased == 0 returns HRS_OK and
 * touches nothing; len > UINT32_MAX or a valid entry > len is HRS_EINVAL with
 * the stripe and location named; the plans are built, with the sibling's
 * HRS_EINVAL / HRS_ETOOMANY; a pattern that reads more than 32 survivors is
 * HRS_EINVAL with the stripe named; only then the device is selected
 * (HRS_EDEVICE for a host-only handle). Argument errors come before any byte is
 * copied.
 * Kernels: batches with at most 4 losses and at most 16 survivors read per
 * stripe, 16-byte aligned bases and all four strides, take
 * batch_ragged_kernel<NOUT, NINB> over the whole 2 KiB windows (no
 * instantiation uses scratch); the row tail, every other shape, unaligned layouts and
 * kernel mode 2 take batch_ragged_bytewise_kernel (hrs_last_kernel names them
 * by the plain batch's tail rule). A batch whose every entry equals len takes
 * the plain call's route in kernel modes 0 and 1 and hrs_last_kernel names
 * that kernel, so always calling the ragged form costs one scan of valid; mode
 * 3 keeps the ragged kernels even then (hrs_set_kernel_mode).
 * Not covered, by design: patterns that read more than 32 survivors (codes
 * with k > 32, which the plain call serves one stripe at a time: HRS_EINVAL
 * here), the JNI overloads and the single-stripe host call. The CRC forms:
 * "ragged repair + CRC-32" below; scrubbing and healing ragged cells: "ragged
 * scrub and heal". */

/* hrs_decode_batch_dev's layout plus valid. Asynchronous on stream; valid is
 * copied before the call returns (in plan order, through the handle's per-call
 * table slots, with the plans) and may be reused at once. */
hrs_status hrs_decode_batch_ragged_dev(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                       size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                       size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                       size_t nstripes, const uint32_t* valid, void* stream);

/* hrs_decode_batch_host's layout plus valid (HOST stripes and out).
 * Synchronous: the outputs' leading bytes are in place when the call returns. */
hrs_status hrs_decode_batch_ragged_host(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                        size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                        size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                        size_t nstripes, const uint32_t* valid);

/* ---- ragged repair + CRC-32: the checksum a repaired block is accepted by ----
 * The reference accepts a repaired block only by its checksum:
 * Decoder.fixErasedBlock makes a fresh CRC32 (Decoder.java:222-229),
 * fixErasedBlockImpl updates it with crc.update(writeBufs[i], 0, toWrite),
 * toWrite = min(bufSize, limit - written) (Decoder.java:360-369), and the
 * value is compared with the stored block checksum. So the checksum of a
 * repaired cell of a file's last stripe covers EXACTLY the cell's real length,
 * with no zero fill behind it. These are the two ragged repair calls above
 * with those CRCs from the same pass; their semantics are the product of the
 * "ragged repair" contract and the "batches + CRC-32" rules, plus one sentence:
 *   - every byte written to out, every byte left untouched, the survivor
 *     choice, HRS_ETOOMANY and the code families are exactly the ragged
 *     sibling's; valid is a HOST uint32_t[nstripes * n] in hops order, free on
 *     return; bytes at or beyond valid never influence an output or a CRC;
 *   - the CRC layout is hrs_decode_batch_crc_dev's, [nstripes * max_erased]:
 *     crc_out[s * max_erased + t] belongs to output t of stripe s;
 *   - with e = erased[s * max_erased + t], crc_out[s * max_erased + t] is the
 *     zlib CRC-32 of the first valid[s * n + e] bytes of the rebuilt cell,
 *     continued from crc_in[s * max_erased + t] (CRC32.update chaining; a NULL
 *     crc_in is a fresh CRC32). NO zeros are appended (Decoder.java:360-369).
 *     This differs on purpose from the ragged ENCODE's CRCs, which follow
 *     Encoder.updateChecksums over the full buffer, zero fill included;
 *   - a length of 0 continues over no bytes: crc_out = crc_in (0 without one);
 *     the same holds for t at or past the stripe's loss count and for every
 *     word of a stripe that lost nothing;
 *   - crc_out may be crc_in itself; any other overlap is HRS_EINVAL.
 * Argument rules, in this order: a NULL handle is HRS_EINVAL with no message;
 * the sibling's argument block (stripes, out, max_erased, erased); with work
 * to do, a NULL crc_out and then the overlap rule, both HRS_EINVAL; a NULL
 * valid is HRS_EINVAL; len == 0, nstripes == 0 or max_erased == 0 returns
 * HRS_OK and touches nothing, the CRC arrays included; len > UINT32_MAX or a
 * valid entry > len is HRS_EINVAL with the stripe and location named; the
 * plans, with the sibling's HRS_EINVAL / HRS_ETOOMANY; a pattern that reads
 * more than 32 survivors is HRS_EINVAL; only then the device is selected
 * (HRS_EDEVICE for a host-only handle). Argument errors come before any byte
 * is copied. hrs_last_kernel / hrs_last_host_path behave as for the sibling;
 * the host path is set only on success.
 * Kernels: batches of at most 4 losses and at most 12 survivors read per
 * stripe (8 at 4 losses), len a multiple of 2 KiB, 16-byte aligned bases and
 * strides, kernel mode 0 or 3, take batch_ragged_crc_kernel<NOUT, NINB, 768>:
 * the ragged repair's walk with the raw CRC of every live output window taken
 * from the registers (the boundary window's words masked from the boundary
 * on; a dead window costs no store, no table lookup and has no raw word; out
 * is never read). Everything else (the row tail, unaligned layouts, more than
 * 4 losses, 13-32 survivors, kernel modes 1 and 2) runs the ragged repair,
 * then crc_ragged_window_kernel over the outputs up to each cell's length
 * (which reads back only bytes the repair just wrote), and hrs_last_kernel
 * names the ragged repair's kernel. batch_ragged_crc_fold_kernel finishes
 * both: it joins the raw words that exist and takes the zero padding of the
 * last word (or of the row) off again, Z_pad being invertible
 * (lambdafs_amd/csrc/crc32.hpp). A batch whose every entry equals len takes
 * hrs_decode_batch_crc_dev's route in kernel modes 0 and 1; mode 3 keeps the
 * ragged kernels even then (hrs_set_kernel_mode).
 * Not covered, by design: the JNI overloads, the single-stripe host call,
 * patterns that read more than 32 survivors, a ragged form of the checked
 * repair (its first stage, the scrub and heal over ragged cells, exists:
 * "ragged scrub and heal" below; its CRC forms and heal-erased do not yet). */

/* hrs_decode_batch_ragged_dev + the CRC-32 of every rebuilt cell over exactly
 * its length. crc_in (nullable) and crc_out are DEVICE arrays of
 * nstripes * max_erased words. Asynchronous on stream. */
hrs_status hrs_decode_batch_ragged_crc_dev(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                           size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                           size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                           size_t nstripes, const uint32_t* valid, const uint32_t* crc_in,
                                           uint32_t* crc_out, void* stream);

/* hrs_decode_batch_ragged_host + the same CRCs; crc_in / crc_out are HOST
 * arrays. Synchronous. */
hrs_status hrs_decode_batch_ragged_host_crc(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                            size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                            size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                            size_t nstripes, const uint32_t* valid, const uint32_t* crc_in,
                                            uint32_t* crc_out);

/* ---- stripe scrubbing: ReedSolomonCode.computeErrorLocations in bulk ----
 * Whether a stripe at rest is still a codeword, and which cells went bad when
 * nothing reported an erasure. For each byte column c of each stripe the
 * column data[l] = rows[l][c], l in [0, n) in hops order, goes through
 * computeErrorLocations (ReedSolomonCode.java:243-287, computeSyndrome
 * :298-307) exactly as the Java runs it, its quirks included: the
 * elimination's row-wise pivot search (GaloisField.java:412-451), no
 * resolvable error at parity_size 1, resolved words with a wrong location set
 * at larger parity sizes. A stripe's report aggregates its columns in
 * HRS_SCRUB_HEAD + n uint32 words:
 *   word 0 HRS_SCRUB_BAD         columns with a nonzero syndrome
 *   word 1 HRS_SCRUB_UNRESOLVED  columns where the method returns false
 *   word 2 HRS_SCRUB_FIRST_BAD   lowest column counted in word 0, or HRS_SCRUB_NONE
 *   word 3                       0 (hrs_heal_*: HRS_SCRUB_PATCHED, below)
 *   word 4 + l                   columns that returned true and whose errorLocations holds l
 * Columns that return false add nothing to words 4... Every word is a count
 * or a minimum: the report does not depend on scheduling. The locations with
 * a nonzero count are the stripe's erasure list for hrs_decode_batch_dev.
 * rs codes with parity_size <= 8 only (HRS_EINVAL otherwise). */
#define HRS_SCRUB_BAD 0
#define HRS_SCRUB_UNRESOLVED 1
#define HRS_SCRUB_FIRST_BAD 2
#define HRS_SCRUB_HEAD 4            /* words before the per-location counts */
#define HRS_SCRUB_NONE 0xFFFFFFFFu

/* ReedSolomonCode.computeErrorLocations on one column, host only (works on
 * HRS_DEVICE_NONE handles). data[n] in [0,255], hops order; mutated as the
 * Java mutates it (:281-285). locations has room for n, filled ascending;
 * *resolved receives the method's boolean. */
hrs_status hrs_compute_error_locations(const hrs_codec* codec, int* data, int* locations, int* num_locations,
                                       int* resolved);

/* Device-resident batch: rows[n] DEVICE pointers of stripe 0 (none NULL),
 * stripe s at rows[l] + s * stride. reports: DEVICE uint32, stripe s at
 * reports + s * report_stride (words, >= 4 + n); its 4 + n words are fully
 * overwritten. 16-byte aligned rows and stride take the vector kernel over
 * the whole 2 KiB windows; the row tail, or everything otherwise, a
 * byte-granular kernel. len == 0 or nstripes == 0: nothing is touched.
 * Asynchronous on stream. */
hrs_status hrs_scrub_dev(hrs_codec* codec, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, void* stream);

/* Same over a HOST batch laid out like hrs_decode_batch_host (stripe s holds
 * location l at stripes + s * stripe_stride + l * row_stride); reports is a
 * HOST array. Runtime-pinned stripes are read in place by one launch, any
 * other memory is staged through the host-batch pipeline. Synchronous.
 * The cells must not overlap (HRS_EINVAL): row_stride >= len, and with more
 * than one stripe stripe_stride >= len and either a stripe's rows lie inside
 * the stripe stride or a row's stripes inside the row stride. */
hrs_status hrs_scrub_batch_host(hrs_codec* codec, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                size_t len, size_t nstripes, uint32_t* reports, size_t report_stride);

/* ---- stripe healing: the scrub plus the write-back, in one pass ----
 * The scalar method patches the column it located (data[loc] = decoded value,
 * ReedSolomonCode.java:281-285); the scrub computes those values and drops
 * them. Heal stores them, under this rule:
 *   - a column for which computeErrorLocations returns true with a non-empty
 *     location set is rewritten to the Java's post-call data; only the bytes
 *     whose error value is nonzero are stored (a blamed location whose value
 *     stands is counted in word 4 + l and not written);
 *   - a column for which it returns false is left exactly as it was, also
 *     where the Java wrote into it before returning false.
 * The report is the scrub's report of the stripes as they were BEFORE the
 * call, except
 *   word 3 HRS_SCRUB_PATCHED     bytes this call stored = bytes that differ
 *                                before and after (hrs_scrub_* keep writing 0)
 * A resolved column with at most parity_size / 2 wrong bytes is always
 * restored to the codeword it came from; beyond that the method usually
 * returns false, and rarely resolves to another codeword (the code's distance
 * limit). Each column is written by the one lane that
 * owns it: the result does not depend on scheduling, and a second heal finds
 * only the unresolved columns and stores nothing. Codes as for the scrub. */
#define HRS_SCRUB_PATCHED 3

/* Device-resident batch, arguments as hrs_scrub_dev; the rows are read and
 * written. No row NULL and no two row pointers equal (HRS_EINVAL: a patch
 * through one would change the other's column). Kernel mode 2 forces the
 * byte-granular kernel. Asynchronous on stream. */
hrs_status hrs_heal_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                        uint32_t* reports, size_t report_stride, void* stream);

/* Same over a HOST batch laid out as for hrs_scrub_batch_host, cell-overlap
 * rule included. Runtime-pinned stripes are healed in place by one launch (the
 * few patched bytes cross the host link); any other memory is staged through
 * the host-batch pipeline, and only the cells whose count in word 4 + l is
 * nonzero are copied back: no other byte of the caller's memory is written.
 * Synchronous. */
hrs_status hrs_heal_batch_host(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                               size_t len, size_t nstripes, uint32_t* reports, size_t report_stride);

/* The same operation for one stripe of n HOST rows on the CPU (works on
 * HRS_DEVICE_NONE handles): a plain loop over the columns through the locator
 * the kernels run. report: 4 + n words. len == 0: nothing is touched. */
hrs_status hrs_heal_host(const hrs_codec* codec, uint8_t* const* rows, size_t len, uint32_t* report);

/* ---- ragged scrub and heal: per-cell lengths, zero tails never read ----
 * The stripes of a file's tail are encoded from short and empty cells (the
 * "ragged encode" above: ReadResult.numRead, ParallelStreamReader.java:236-249)
 * and repaired up to the lost block's real length (the "ragged repair":
 * Decoder.java:345-369). Their zero tails are stored nowhere. These calls are
 * hrs_scrub_dev, hrs_heal_dev, hrs_scrub_batch_host, hrs_heal_batch_host and
 * hrs_heal_host plus one number per cell, so that scrubbing data at rest reads
 * none of those zeros either:
 *   - valid is a HOST array of uint32_t[nstripes * n] in hops order, as for the
 *     ragged repair; valid[s * n + l] is the length of cell l of stripe s, and
 *     the cell counts as those bytes followed by len - valid zeros.
 * Column c of stripe s is data[l] = c < valid[s * n + l] ? rows[l][c] : 0, and
 * computeErrorLocations runs on it exactly as the siblings run it, every quirk
 * of the reference kept. The report layout is the scrub's, 4 + n words;
 * HRS_SCRUB_PATCHED is counted by the heal calls only. The calls guarantee:
 *   - bytes at or beyond a cell's valid never influence a report or a stored
 *     byte, whatever they hold, and are never written; the storage of the
 *     whole cell (len bytes) must still be addressable;
 *   - one rule beyond the siblings', DEMOTION: a virtual zero cannot be
 *     patched. A column is demoted when the method returns true, blames a
 *     location l with a nonzero error value, and c >= valid[s * n + l]. A
 *     demoted column counts as unresolved: word 1, not words 4 + l (words 0
 *     and 2 count it as usual). Heal stores nothing in a demoted column, also
 *     not the errors it resolved in live cells of the same column: a
 *     half-patched column is not a codeword. Scrub and heal apply the same
 *     rule, so heal's report is still the ragged scrub's report of the stripes
 *     before the call, plus word 3. A blamed location whose error value is 0
 *     (the parity_size 8 quirk) demotes nothing.
 *     A demoted column means: the lengths disagree with the bytes the parity
 *     was made from (a cell recorded shorter than the data that was encoded);
 *   - if no column of a batch is demoted, the report equals hrs_scrub_dev's
 *     over the zero-filled stripes and heal's bytes below valid equal
 *     hrs_heal_dev's; a batch whose every entry equals len equals the plain
 *     calls word for word (nothing can be demoted there);
 *   - the vector kernel loads no 2 KiB window of a cell that lies wholly at or
 *     beyond the cell's valid, loads and masks the one window that holds the
 *     boundary, and loads nothing at all for a window at or beyond every
 *     cell's length of that stripe;
 *   - the staged host path copies in no byte at or beyond valid and, after a
 *     heal, copies back only the cells whose word 4 + l is nonzero, and of
 *     those only the first valid bytes (with HRS_ZEROCOPY=0 no byte at or
 *     beyond valid is sent to or fetched from the device); runtime-pinned
 *     batches run as one zero-copy launch in place.
 * Argument rules, in this order, all before any byte is copied: a NULL handle
 * is HRS_EINVAL with no message; the sibling's argument rules (code, reports,
 * rows; heal keeps its NULL-row and equal-rows rule, the host batches their
 * overlapping-cells rule); a NULL valid is HRS_EINVAL; len == 0 or
 * nstripes == 0 returns HRS_OK and touches nothing; a valid entry > len is
 * HRS_EINVAL with the stripe and location named; only then the device is
 * selected (HRS_EDEVICE for a host-only handle). valid is copied before the
 * device calls return (through the handle's per-call table slots) and may be
 * reused at once. Codes as for the scrub: rs, parity_size <= 8, any n <= 255.
 * Kernels: 16-byte aligned rows and stride take scrub_ragged_kernel<P> /
 * heal_ragged_kernel<P> over the whole 2 KiB windows (no instantiation uses
 * scratch); the row tail, unaligned rows or strides and kernel mode 2 take
 * scrub_ragged_bytewise_kernel<P> / heal_ragged_bytewise_kernel<P>, which load
 * a location's byte only where the column lies below its length. A batch whose
 * every entry equals len takes the plain call's route in kernel modes 0 and 1
 * and hrs_last_kernel names that kernel, so always calling the ragged form
 * costs one scan of valid; mode 3 keeps the ragged kernels even then
 * (hrs_set_kernel_mode).
 * Out of scope, by design: the CRC forms, heal with known erasures, the checked
 * repair and the JNI overloads over ragged cells. */

/* hrs_scrub_dev's arguments plus valid. Asynchronous on stream. */
hrs_status hrs_scrub_ragged_dev(hrs_codec* codec, const uint8_t* const* rows, size_t stride, size_t len,
                                size_t nstripes, const uint32_t* valid, uint32_t* reports, size_t report_stride,
                                void* stream);

/* hrs_heal_dev's arguments plus valid; the rows are read and, below valid,
 * written. Asynchronous on stream. */
hrs_status hrs_heal_ragged_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const uint32_t* valid, uint32_t* reports, size_t report_stride, void* stream);

/* hrs_scrub_batch_host's layout plus valid (HOST stripes and reports). Synchronous. */
hrs_status hrs_scrub_ragged_batch_host(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                       size_t stripe_stride, size_t len, size_t nstripes, const uint32_t* valid,
                                       uint32_t* reports, size_t report_stride);

/* hrs_heal_batch_host's layout plus valid. Synchronous. */
hrs_status hrs_heal_ragged_batch_host(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                      size_t len, size_t nstripes, const uint32_t* valid, uint32_t* reports,
                                      size_t report_stride);

/* hrs_heal_host plus valid[n]: one stripe of n HOST rows on the CPU (works on
 * HRS_DEVICE_NONE handles), the kernels' byte-exact reference, demotion
 * included. */
hrs_status hrs_heal_ragged_host(const hrs_codec* codec, uint8_t* const* rows, size_t len, const uint32_t* valid,
                                uint32_t* report);

/* ---- heal with known erasures: repair lost cells and fix survivors ----
 * hrs_decode_batch_dev rebuilds lost cells from survivors it trusts blindly;
 * hrs_heal_dev fixes silent errors only while all n cells are present. RS(k,p)
 * corrects e known erasures and t unknown errors of a column whenever
 * e + 2 t <= p, and this call does both in one pass. Per byte column, with E
 * the stripe's erased locations (e <= p, distinct, taken ascending) and
 * d_l the bytes of the survivors l not in E (bytes stored at erased locations
 * are never read):
 *   1. S_i = sum_{l not in E} alpha^(i l) d_l, i < p (erased cells count as 0);
 *   2. Gamma(x) = prod_{m in E} (1 + alpha^m x) = sum_j Gamma_j x^j and
 *      T_i = sum_{j <= e} Gamma_j S_{i+e-j}, i < p' = p - e: the erased cells
 *      add nothing to T, an error u at survivor y adds
 *      u prod_{m in E} (alpha^y + alpha^m) alpha^(y i);
 *   3. every T_i zero, or p' = 0: the survivors are consistent, nobody is blamed;
 *   4. otherwise the column is bad: unresolved if p' < 2, else the locator of
 *      computeErrorLocations (quirks included) runs on the p' values T; the
 *      column is resolved when it returns true and blames no erased location,
 *      and then S is corrected by the errors u_j = err'_j / prod_m (alpha^loc_j + alpha^m);
 *   5. the erased values v solve sum_{m in E} v_m alpha^(m i) = S_i, i < e,
 *      over the corrected S of a resolved column and S as it stands otherwise.
 * Stores: every byte of every erased cell is written with v_m, in every
 * column; in a resolved column each survivor with u_j != 0 gets ^= u_j (the
 * heal's rule: a blamed location whose value stands is counted, not stored);
 * in an unresolved column no survivor is touched, its erased bytes are the
 * solve over the uncorrected syndromes (defined by this rule, NOT claimed to
 * equal hrs_decode_batch_dev's bytes there) and it is counted in word 1.
 * Report, the heal's layout, 4 + n words per stripe:
 *   word 0 HRS_SCRUB_BAD         columns with a nonzero T
 *   word 1 HRS_SCRUB_UNRESOLVED  unresolved columns
 *   word 2 HRS_SCRUB_FIRST_BAD   lowest bad column, or HRS_SCRUB_NONE
 *   word 3 HRS_SCRUB_PATCHED     survivor bytes stored (the fill of the
 *                                erased cells is not counted)
 *   word 4 + l                   resolved columns that blamed survivor l
 *                                (always 0 for l in E)
 * Every word is a count or a minimum: scheduling cannot change it.
 * Three properties follow:
 *   - e = 0: T = S and Gamma = 1; the call equals hrs_heal_dev byte for byte
 *     and report word for report word;
 *   - consistent survivors: the erased cells equal hrs_decode_batch_dev's
 *     output rows (any k consistent survivors give the same codeword), the
 *     survivors are unchanged and the report is empty;
 *   - uniqueness: if the survivors differ from a codeword c in t <= p' / 2
 *     places and the column comes back resolved, all n bytes equal c: the
 *     result is a codeword within p' / 2 survivor places of the stored word,
 *     c is within t of it, and two codewords that differ in at most p'
 *     survivor places plus e erased places (<= p < p + 1) are one codeword. A
 *     resolved column within capacity is never miscorrected.
 * Whether a column within capacity always resolves is the reference
 * locator's business: it does at parity_size <= 4; at parity_size 8 the
 * quirky elimination leaves a few such columns unresolved (DESIGN.md section
 * 10.3). Past capacity the distance limit holds as for the heal; at e = p no
 * spare is left and every error goes undetected. A caller who cannot accept
 * that takes the cells' CRCs from the same call (hrs_heal_erased_crc_dev,
 * hrs_heal_erased_batch_host_crc below) and compares them with the stored
 * checksums. Codes as for the scrub. */

/* Device-resident batch. rows, stride, len, nstripes, reports, report_stride
 * and stream as for hrs_heal_dev (n DEVICE pointers, none NULL, no two equal;
 * cells at erased locations are written, never read). erased: HOST int array
 * laid out as for hrs_decode_batch_dev, the erased locations of stripe s at
 * erased[s * max_erased + t] up to the first negative value (or max_erased
 * entries); a stripe may have none. More than parity_size erasures in a
 * stripe: HRS_ETOOMANY; a location outside [0, n), a location repeated within
 * a stripe or max_erased < 0: HRS_EINVAL. Argument errors come before the
 * device is selected (HRS_EDEVICE for a host-only handle). len == 0 or
 * nstripes == 0 touches nothing; max_erased == 0 is hrs_heal_dev. The
 * stripes' erasure sets are de-duplicated into a device table (any number of
 * distinct patterns). 16-byte aligned rows and stride take
 * heal_erased_kernel<P> over the whole 2 KiB windows (every parity size 1..8
 * is built without scratch memory; none is routed away); the row tail,
 * unaligned layouts and kernel mode 2 take heal_erased_bytewise_kernel<P>
 * (hrs_last_kernel names them by the scrub's tail rule). Asynchronous on
 * stream. */
hrs_status hrs_heal_erased_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                               void* stream);

/* The same operation for one stripe of n HOST rows on the CPU (works on
 * HRS_DEVICE_NONE handles): a plain loop over the columns through the locator
 * the kernels run, their byte-exact reference. erased[num_erased]: the
 * stripe's erased locations (read up to the first negative value). report:
 * 4 + n words. len == 0: nothing is touched. */
hrs_status hrs_heal_erased_host(const hrs_codec* codec, uint8_t* const* rows, size_t len, const int* erased,
                                int num_erased, uint32_t* report);

/* ---- scrub and heal + CRC-32: the block checksums in the same pass ----
 * In the reference system a bad cell is first known by its block checksum
 * (Encoder.java:408-450 stores one per block; Decoder.java:373-387 turns a
 * ChecksumException into an erased location), and a checksum mismatch names
 * up to parity_size bad cells where the syndromes stop at parity_size / 2;
 * the syndromes in turn see a stale parity cell whose checksum was rewritten
 * with it. These are the four scrub / heal calls above with the CRC-32 of
 * every cell computed from the same read. The common rules of "batches +
 * CRC-32" hold (chaining from crc_in, NULL crc_in = fresh, crc_out may be
 * crc_in itself and any other overlap is HRS_EINVAL, a NULL crc_out with work
 * to do is HRS_EINVAL, len == 0 or nstripes == 0 touches nothing, argument
 * errors before the device, HRS_EDEVICE for a host-only handle), and:
 *  - crc_out[s * n + l] belongs to hops location l of stripe s: HOPS ORDER,
 *    parity first, the order of rows[] - NOT the data-first order of
 *    hrs_encode_crc_dev and hrs_encode_batch_host_crc;
 *  - scrub: the CRCs cover the cells as read; nothing is written to them;
 *  - heal: the CRCs cover the cells as they are when the call returns, after
 *    the write-back: the value to compare with the stored checksum to decide
 *    whether the heal restored the block (an unresolved column is left as it
 *    was and its cell's CRC says so);
 *  - reports, the bytes healed, the bytes left untouched and every argument
 *    rule are exactly the sibling call's.
 * rs codes with 2 <= parity_size <= 4 and n <= 16, len a multiple of 2 KiB,
 * 16-byte aligned rows and stride, kernel mode 0 or 3 take one fused kernel
 * (hrs_last_kernel "scrub_crc_kernel<P>" / "heal_crc_kernel<P>"; the heal
 * re-reads only the 2 KiB windows it patched); anything else runs the sibling
 * call, then the CRC pass over the n rows, with identical results (and
 * hrs_last_kernel as the sibling reports it). */

/* hrs_scrub_dev + the CRCs. crc_in / crc_out: DEVICE uint32 [nstripes * n].
 * Asynchronous on stream. */
hrs_status hrs_scrub_crc_dev(hrs_codec* codec, const uint8_t* const* rows, size_t stride, size_t len,
                             size_t nstripes, uint32_t* reports, size_t report_stride, const uint32_t* crc_in,
                             uint32_t* crc_out, void* stream);

/* hrs_heal_dev + the CRCs of the cells after the write-back. */
hrs_status hrs_heal_crc_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                            uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                            void* stream);

/* hrs_scrub_batch_host + the CRCs; crc_in / crc_out are HOST uint32
 * [nstripes * n] (read before the first chunk, written once after the last).
 * Runtime-pinned stripes of a fused shape cross the host link once.
 * Synchronous. */
hrs_status hrs_scrub_batch_host_crc(hrs_codec* codec, const uint8_t* stripes, size_t row_stride,
                                    size_t stripe_stride, size_t len, size_t nstripes, uint32_t* reports,
                                    size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out);

/* hrs_heal_batch_host + the CRCs of the cells after the write-back; staged
 * cells go back to the caller exactly as for hrs_heal_batch_host. */
hrs_status hrs_heal_batch_host_crc(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                   size_t len, size_t nstripes, uint32_t* reports, size_t report_stride,
                                   const uint32_t* crc_in, uint32_t* crc_out);

/* ---- heal with known erasures over host batches, and with block CRC-32s ----
 * hrs_heal_erased_dev for stripes in HOST memory, and both forms with the
 * CRC-32 of every cell from the same call. Nothing new is defined: bytes,
 * reports, the erased list's rules (HOST int array, read up to the first
 * negative entry per stripe; HRS_ETOOMANY above parity_size locations with the
 * stripe named; HRS_EINVAL for a location out of range, a repeated one or
 * max_erased < 0) and codes (rs, parity_size <= 8) are hrs_heal_erased_dev's,
 * and max_erased == 0 is the corresponding heal call (hrs_heal_crc_dev,
 * hrs_heal_batch_host, hrs_heal_batch_host_crc). Argument errors, the erased
 * list's included, come before the device is selected and before any byte is
 * copied; valid arguments on a host-only handle are HRS_EDEVICE; len == 0 or
 * nstripes == 0 touches nothing, the CRC arrays included.
 *
 * CRCs follow the rules of "scrub and heal + CRC-32": crc_out[s * n + l] is
 * the CRC-32 of hops location l of stripe s, HOPS ORDER, continued from
 * crc_in (NULL = fresh); crc_out may be crc_in itself, any other overlap and a
 * NULL crc_out with work to do are HRS_EINVAL. They cover the cells as they
 * are when the call returns: rebuilt cells, patched survivors, and unresolved
 * columns as left. A caller compares them with the stored checksums to accept
 * the stripe, which also covers what the distance limit lets through.
 *
 * rs codes with 2 <= parity_size <= 4 and n <= 16, len a multiple of 2 KiB,
 * 16-byte aligned rows and stride have one fused kernel
 * (hrs_last_kernel "heal_erased_crc_kernel<P>": the survivors are read once,
 * only the 2 KiB windows with a bad column are read again). Kernel mode 3
 * always takes it for such a shape, kernel mode 2 never; kernel mode 0 takes
 * it where it was measured faster than two passes for the memory the stripes
 * lie in. Everything else runs hrs_heal_erased_dev's
 * kernels, then the CRC pass over the n rows on the same stream, with
 * identical results and hrs_last_kernel as the sibling reports it. */

/* hrs_heal_erased_dev + the CRCs. crc_in / crc_out: DEVICE uint32
 * [nstripes * n]. Asynchronous on stream. */
hrs_status hrs_heal_erased_crc_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                   const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                                   const uint32_t* crc_in, uint32_t* crc_out, void* stream);

/* hrs_heal_erased_dev over a HOST batch laid out as for hrs_heal_batch_host,
 * cell-overlap rule included; reports is a HOST array. Runtime-pinned stripes
 * are healed in place by one launch: erased cells never cross the link
 * inbound. Any other memory is staged through the host-batch pipeline: of a
 * stripe only its survivor rows are copied in, and only its erased cells
 * (fully written, never read) and the cells with a nonzero count in word
 * 4 + l are copied back: no other byte of the caller's memory is written.
 * hrs_last_host_path as for the sibling calls. Synchronous. */
hrs_status hrs_heal_erased_batch_host(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                      size_t len, size_t nstripes, const int* erased, int max_erased,
                                      uint32_t* reports, size_t report_stride);

/* hrs_heal_erased_batch_host + the CRCs; crc_in / crc_out are HOST uint32
 * [nstripes * n] (read before the first chunk, written once after the last). */
hrs_status hrs_heal_erased_batch_host_crc(hrs_codec* codec, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                          size_t len, size_t nstripes, const int* erased, int max_erased,
                                          uint32_t* reports, size_t report_stride, const uint32_t* crc_in,
                                          uint32_t* crc_out);

/* ---- checked repair: stored checksums in, verdicts out ----
 * The workflow of the reference's Decoder and BlockReconstructor as one call:
 * a cell is first known to be bad by its block checksum (Decoder.java:373-387),
 * it becomes an erased location, the stripe is repaired, and the repaired
 * block is accepted by its checksum (Decoder.java:222-229, :645-655). Per
 * stripe, with C_l the CRC-32 of cell l as read, stored_l the caller's
 * checksum of it and R the stripe's hrs_scrub_dev report:
 *   1. D = { l : C_l != stored_l };
 *   2. B = D, or with HRS_REPAIR_JOIN_SYNDROMES B = D + { l : R[4 + l] != 0 };
 *   3. in this order: D empty and R[1] > 0: HRS_REPAIR_AMBIGUOUS (unresolved
 *      columns and no checksum differs); D empty and R[0] = 0:
 *      HRS_REPAIR_CLEAN; |B| > parity_size: HRS_REPAIR_TOOMANY; otherwise the
 *      stripe is listed with the erasure set E = B (E may be empty: without
 *      the join flag, D empty, R[0] > 0 and R[1] = 0 runs the plain heal);
 *   4. a clean, too-many or ambiguous stripe is never written and the second
 *      pass never reads it: its report is R, its crc_out words are C, its
 *      erased_out row is all -1;
 *   5. a listed stripe gets exactly hrs_heal_erased_dev's bytes and report for
 *      E; its erased_out row holds E ascending, -1 padded, and its crc_out
 *      words the CRCs of the cells as the call leaves them;
 *   6. with F = { l : crc_out_l != stored_l } and R' the listed stripe's
 *      report: F empty: HRS_REPAIR_REPAIRED; F and D disjoint and R'[1] = 0:
 *      HRS_REPAIR_RESTAMP (the stripe is a codeword and every checksum that
 *      was doubted now matches; the cells in F held a matching checksum over
 *      stale bytes, and crc_out has their new values); anything else:
 *      HRS_REPAIR_FAILED, the bytes as hrs_heal_erased_dev leaves them.
 * Every output is a function of the inputs alone. Checksums alone (flags 0)
 * is the reference's rule and the default: a cell of whole-cell garbage puts
 * more errors into every column than the locator resolves, the few columns it
 * then mis-resolves blame cells that are sound, and the joined set can pass
 * parity_size for damage that is inside the code's capacity (DESIGN.md
 * section 10.5). The join flag is for few-column damage whose checksum was
 * rewritten with it. Codes as for the scrub. */
#define HRS_REPAIR_JOIN_SYNDROMES 1 /* flags bit 0 */
enum {
  HRS_REPAIR_CLEAN = 0,
  HRS_REPAIR_REPAIRED = 1,
  HRS_REPAIR_RESTAMP = 2,
  HRS_REPAIR_FAILED = 3,
  HRS_REPAIR_TOOMANY = 4,
  HRS_REPAIR_AMBIGUOUS = 5
};

/* Device-resident batch. rows, stride, len, nstripes, reports, report_stride
 * and stream as for hrs_heal_erased_dev (n DEVICE pointers in hops order, none
 * NULL, no two equal). DEVICE arrays: stored, uint32 [nstripes * n], the fresh
 * whole-cell CRC-32s in hops order like hrs_scrub_crc_dev's crc_out (there is
 * no crc_in); crc_out, the same shape, which must not overlap stored
 * (HRS_EINVAL); verdicts, uint32 [nstripes]; erased_out, int32
 * [nstripes * parity_size], may be NULL. A flags bit other than bit 0 is
 * HRS_EINVAL, and so is a NULL stored, verdicts, reports or crc_out with work
 * to do. Argument errors come first; then len == 0 or nstripes == 0 returns
 * HRS_OK and touches nothing; then the device is selected (HRS_EDEVICE for a
 * host-only handle). Any alignment is accepted, by the siblings' split: vector
 * kernels over the whole 2 KiB windows, byte-granular kernels over tails,
 * unaligned layouts and kernel mode 2.
 *
 * Everything runs on stream with no host wait, no copy to the host and no
 * host-built table between the passes: pass 1 is hrs_scrub_crc_dev as it is
 * (hrs_last_kernel names its kernel); repair_plan_kernel applies steps 1-3,
 * builds each listed stripe's erasure pattern on the device and appends the
 * stripe to a list in the handle's scratch; pass 2 (heal_listed_kernel<P>,
 * heal_listed_bytewise_kernel<P>: hrs_heal_erased_dev's kernels over the
 * listed stripes only), the CRC pass and the verdicts take their task range
 * from that list. The scratch holds one table entry of 128 bytes and one list
 * word per stripe of the batch beside the raw window CRCs of pass 1.
 * Asynchronous on stream. */
hrs_status hrs_repair_checked_dev(hrs_codec* codec, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                  const uint32_t* stored, int flags, uint32_t* verdicts, int32_t* erased_out,
                                  uint32_t* reports, size_t report_stride, uint32_t* crc_out, void* stream);

/* The same operation for one stripe of n HOST rows on the CPU (works on
 * HRS_DEVICE_NONE handles), the device call's byte-exact reference: the
 * locator loop of hrs_heal_host and hrs_heal_erased_host and a host CRC-32
 * under the same rule (one header compiled by both). stored, crc_out: n
 * words; verdict: one word; erased_out: parity_size words or NULL; report:
 * 4 + n words. len == 0: nothing is touched. */
hrs_status hrs_repair_checked_host(const hrs_codec* codec, uint8_t* const* rows, size_t len, const uint32_t* stored,
                                   int flags, uint32_t* verdict, int32_t* erased_out, uint32_t* report,
                                   uint32_t* crc_out);

/* Kernel selection for tests and benchmarks: 0 = auto (default), 1 = force
 * the runtime-matrix bit-sliced kernel, 2 = force the byte-granular kernel,
 * 3 = auto, except that hrs_encode_crc_dev and the heal-with-erasures + CRC
 * calls take their fused kernel whenever the shape allows it.
 * The ragged encode calls: 0 and 1 send a batch whose every valid entry equals
 * len to the plain encode (which then follows its own mode) and any other
 * batch to the ragged kernels, vector where the shape has one; 2 forces
 * encode_ragged_bytewise_kernel for every batch; 3 keeps the ragged kernels
 * for an all-full batch too (tests and benchmarks).
 * The ragged encode + CRC calls: 0 and 1 send an all-full batch to
 * hrs_encode_crc_dev's route (which then follows its own mode); for any other
 * batch 0 and 3 take encode_ragged_crc_kernel where the shape has one, 1 and 2
 * never fuse (ragged encode, crc_ragged_window_kernel, fold), 2 with the
 * byte-granular encode; 3 keeps the ragged kernels for an all-full batch too.
 * The ragged repair calls: 0 and 1 send a batch whose every valid entry equals
 * len to the plain batch's route (which then follows its own mode) and any
 * other batch to the ragged kernels, batch_ragged_kernel where the shape has
 * one; 2 forces batch_ragged_bytewise_kernel for every batch; 3 keeps the
 * ragged kernels for an all-full batch too.
 * The ragged repair + CRC calls: 0 and 1 send an all-full batch to
 * hrs_decode_batch_crc_dev's route with the plans already built (the CRC over
 * len bytes then is the CRC over valid bytes); for any other batch 0 and 3
 * take batch_ragged_crc_kernel where the shape has one, 1 and 2 never fuse
 * (ragged repair, crc_ragged_window_kernel over the outputs, fold), 2 with
 * the byte-granular repair; 3 keeps the ragged kernels for an all-full batch
 * too. With nothing lost anywhere only the fold runs.
 * The ragged scrub and heal calls: 0 and 1 send a batch whose every valid
 * entry equals len to the plain call's route (hrs_last_kernel names
 * scrub_kernel / heal_kernel) and every other batch to the ragged kernels; 2
 * forces scrub_ragged_bytewise_kernel / heal_ragged_bytewise_kernel for every
 * batch; 3 keeps the ragged kernels for an all-full batch too. */
hrs_status hrs_set_kernel_mode(hrs_codec* codec, int mode);

#ifdef __cplusplus
}
#endif

#endif /* HRS_H_ */
