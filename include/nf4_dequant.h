/*
 * nf4_dequant.h -- C ABI of the MI355X (gfx950) NF4 double-dequantization path.
 *
 * Library: nf4_triton_dequantization_amd/_lib/libnf4dq.so (hipcc, gfx950).
 * Every entry point is asynchronous on the given HIP stream, allocates nothing,
 * keeps no global mutable state, and returns 0 or an NF4DQ_* error code.
 * Pointers are device pointers unless stated otherwise; `hip_stream` is a
 * hipStream_t (NULL = the null stream).
 *
 * Reference interfaces replaced (felipemcoelho/nf4-triton-dequantization,
 * file nf4_triton_dequantization/kernel_optimized.py):
 *   nf4_dequant_ref    <- _triton_dequantize_main :142-205 launching
 *                         _nf4_dequantize_kernel_final :11-110 (uint8 absmax,
 *                         double dequant; wrap/truncate rules :173-186)
 *   nf4_dequant_single <- the non-uint8 absmax branch :166-167 -> :273-274
 *   nf4_dequant_ref_batched <- benchmark.py:68-84 (several Linear4bit weights
 *                         per step) folded into one launch
 *   nf4_dequant_ref_cpu / nf4_dequant_single_cpu <- _aggressive_pytorch_t4
 *                         :208-314, the reference's CPU path (HOST pointers,
 *                         synchronous, `threads` worker threads)
 *   nf4_dequant_bnb / nf4_dequant_bnb_single <- bitsandbytes dequantize_4bit
 *                         semantics; the reference
 *                         never implements these, they are parity-unpinned.
 */
#ifndef NF4_DEQUANT_H_
#define NF4_DEQUANT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Output dtypes (quant_state.dtype, kernel_optimized.py:123, :189). */
#define NF4DQ_F16 0
#define NF4DQ_BF16 1
#define NF4DQ_F32 2

/* Return codes. HIP launch failures are NF4DQ_ERR_HIP_BASE + hipError_t. */
#define NF4DQ_OK 0
#define NF4DQ_ERR_ARG 1        /* null pointer, bad dtype, negative size      */
#define NF4DQ_ERR_SHAPE 2      /* sizes the reference would reject (view fails) */
#define NF4DQ_ERR_TOO_LARGE 3  /* a single matrix beyond 2^31 packed bytes    */
#define NF4DQ_ERR_SPLITK_TIMEOUT 4 /* nf4_gemm_check_workspace: a split-K reducer gave up */
#define NF4DQ_ERR_HIP_BASE 1000

/* Reference double dequant of one Linear4bit weight into row-major out[m][n].
 *   packed   uint8[packed_len]  two NF4 codes per byte, high nibble first;
 *                               row r starts at r*(packed_len/m)
 *   absmax_q uint8[nb]          per (row, 64-column block); index wraps mod nb
 *   absmax2  fp32[n2]           index r*ceil(bpr/4) + block/4, wraps mod n2
 * out[r][c] = RNE(NF4[nib] * ((float)absmax_q[.] / 127.0f * absmax2[.])).
 * Errors: packed_len % m != 0 or packed_len/m < ceil(n/2) -> NF4DQ_ERR_SHAPE.
 *
 * Departure from SURVEY.md §8(b): the survey's contract is
 *   nf4_dequant_ref(packed, absmax_q, nb, absmax2, n2, out, out_dtype, m, n, hip_stream);
 * this entry (and nf4_dequant_ref_cpu, nf4_dequant_single, nf4_dequant_single_cpu)
 * adds `packed_len` right after `packed`.  The reference reads the packed weight as
 * `weight.data.view(m, -1)` (kernel_optimized.py:229), so the row stride is
 * numel / m -- padded rows and odd widths included (:288-312) -- and a pointer
 * alone does not carry numel.  Without it the ABI could only assume the dense
 * stride ceil(n/2) and would silently misread padded weights the reference
 * accepts; with it, sizes the reference's view would reject are NF4DQ_ERR_SHAPE. */
int nf4_dequant_ref(const uint8_t* packed, int64_t packed_len,
                    const uint8_t* absmax_q, int64_t nb,
                    const float* absmax2, int64_t n2,
                    void* out, int32_t out_dtype, int64_t m, int64_t n,
                    void* hip_stream);

/* Single-quant branch: absmax fp32[absmax_len] viewed as [m, absmax_len/m],
 * scale of (r, b) = absmax[r*(absmax_len/m) + b]. */
int nf4_dequant_single(const uint8_t* packed, int64_t packed_len,
                       const float* absmax, int64_t absmax_len,
                       void* out, int32_t out_dtype, int64_t m, int64_t n,
                       void* hip_stream);

/* Host-CPU forms of nf4_dequant_ref / nf4_dequant_single:
 * same arguments, same semantics bit for bit, same error codes, but every
 * pointer is a HOST pointer and the call is synchronous; `threads` worker
 * threads split the rows (<= 0 = all hardware threads).  AVX2 table lookups
 * when the CPU has AVX2, a scalar loop otherwise (same results).  Replaces the
 * reference's CPU fallback _aggressive_pytorch_t4 (kernel_optimized.py:208-314). */
int nf4_dequant_ref_cpu(const uint8_t* packed, int64_t packed_len,
                        const uint8_t* absmax_q, int64_t nb,
                        const float* absmax2, int64_t n2,
                        void* out, int32_t out_dtype, int64_t m, int64_t n,
                        int32_t threads);
int nf4_dequant_single_cpu(const uint8_t* packed, int64_t packed_len,
                           const float* absmax, int64_t absmax_len,
                           void* out, int32_t out_dtype, int64_t m, int64_t n,
                           int32_t threads);

/* One matrix of a batched call (host memory; copied into kernel arguments). */
typedef struct nf4_matrix_desc {
    const uint8_t* packed;
    int64_t packed_len;
    const uint8_t* absmax_q;
    int64_t nb;
    const float* absmax2;
    int64_t n2;
    void* out;
    int64_t m;
    int64_t n;
} nf4_matrix_desc;

/* Dequantize `count` matrices (same out_dtype) with as few launches as the
 * kernel-argument budget allows (NF4DQ_BATCH_MAX matrices per launch). */
#define NF4DQ_BATCH_MAX 24
int nf4_dequant_ref_batched(const nf4_matrix_desc* descs, int32_t count,
                            int32_t out_dtype, void* hip_stream);

/* bitsandbytes nested semantics over the flat element stream:
 *   absmax_f32[i] = code2[absmax_q[i]] * absmax2[i / blocksize2] + offset
 *   out[k]        = RNE(NF4[nib(k)] * absmax_f32[k / blocksize])
 * blocksize and blocksize2 must be powers of two, blocksize >= 64. */
int nf4_dequant_bnb(const uint8_t* packed, const uint8_t* absmax_q, int64_t nb,
                    const float* code2, const float* absmax2, int64_t n2,
                    float offset, void* out, int32_t out_dtype, int64_t numel,
                    int32_t blocksize, int32_t blocksize2, void* hip_stream);

/* bitsandbytes single-level (compress_statistics=False): fp32 absmax per block. */
int nf4_dequant_bnb_single(const uint8_t* packed, const float* absmax, int64_t nabs,
                           void* out, int32_t out_dtype, int64_t numel,
                           int32_t blocksize, void* hip_stream);

/* Embedding lookup from an NF4 table in bitsandbytes semantics (bnb.nn.Embedding4bit):
 * the weight is the flat stream nf4_dequant_bnb reads, viewed as [rows][dim], and
 *   out[i][j] = the value nf4_dequant_bnb / nf4_dequant_bnb_single writes for element
 *               ids[i] * dim + j, bit for bit (fp16 / bf16 / fp32 `out_dtype`),
 * for i < count: out is a dense [count][dim].  Only the selected rows' packed bytes and
 * statistics are read.  A row is not a unit of the layout: any dim >= 1 is taken (statistics
 * blocks may span rows, odd rows of an odd dim start on a low nibble); dim % 64 == 0 with
 * `packed` 4-byte and `out` 16-byte aligned runs the fast kernel, anything else an exact
 * one-thread-per-element kernel.
 *   ids     int32 (NF4DQ_IDS_I32) or int64 (NF4DQ_IDS_I64) [count], on the device.
 *           Out-of-range rule: an id outside [0, rows), compared in its own signed type,
 *           gives a row of zero bits and reads nothing from the table -- no device assert,
 *           no out-of-bounds read, no host check (which would synchronise).
 *   offset  ONE fp32 ON THE DEVICE, read when the kernel runs (no host copy, no
 *           synchronisation; it may change between calls); NULL = 0.  As nf4_gemm_bnb.
 *   code2   256 fp32 on the device.
 * blocksize: a power of two, 64..4096; blocksize2: a power of two >= 4; a bad ids_dtype /
 * out_dtype / block size, or a null ids / packed / statistics / out with count > 0:
 * NF4DQ_ERR_ARG (so is a pointer not aligned to its element).  A negative count / rows /
 * dim / nb / n2, dim < 1 with count > 0, nb (nabs) < ceil(rows*dim / blocksize) or n2 <
 * ceil(that / blocksize2): NF4DQ_ERR_SHAPE.  count == 0: NF4DQ_OK, nothing launched.
 * Too-large rule: a call is one launch that indexes its output with 32 bits, so count * dim
 * > 2^31 - 1 is NF4DQ_ERR_TOO_LARGE (never split into several launches; the caller splits
 * `ids`), and so is a table of more than 2^62 elements.
 * One launch on `hip_stream`, no allocation, no read-back: capturable in a graph. */
#define NF4DQ_IDS_I32 0
#define NF4DQ_IDS_I64 1
int nf4_embedding_bnb(const void* ids, int32_t ids_dtype, int64_t count,
                      const uint8_t* packed, const uint8_t* absmax_q, int64_t nb, const float* code2,
                      const float* absmax2, int64_t n2, const float* offset,
                      int32_t blocksize, int32_t blocksize2,
                      void* out, int32_t out_dtype, int64_t rows, int64_t dim, void* hip_stream);
int nf4_embedding_bnb_single(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                             const float* absmax, int64_t nabs, int32_t blocksize,
                             void* out, int32_t out_dtype, int64_t rows, int64_t dim, void* hip_stream);

/* Host forms: every pointer (`offset` included) is a HOST pointer, the call is synchronous,
 * `threads` workers split the output rows (<= 0 = all hardware threads); the same results
 * bit for bit, the same rules and error codes. */
int nf4_embedding_bnb_cpu(const void* ids, int32_t ids_dtype, int64_t count,
                          const uint8_t* packed, const uint8_t* absmax_q, int64_t nb, const float* code2,
                          const float* absmax2, int64_t n2, const float* offset,
                          int32_t blocksize, int32_t blocksize2,
                          void* out, int32_t out_dtype, int64_t rows, int64_t dim, int32_t threads);
int nf4_embedding_bnb_single_cpu(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                                 const float* absmax, int64_t nabs, int32_t blocksize,
                                 void* out, int32_t out_dtype, int64_t rows, int64_t dim, int32_t threads);

/* The producer side: quantize a flat stream of `numel` float elements (`in_dtype`:
 * NF4DQ_F16 / NF4DQ_BF16 / NF4DQ_F32 name the INPUT type here) into the layout the
 * nf4_dequant_bnb* entries read.  The specification is the package's Python quantizer
 * (bnb_layout.quantize_nf4), bit for bit:
 *   absmax[b] = max |x| over block b in fp32 (elements past numel read as 0)
 *   q         = x / (absmax[b] > 0 ? absmax[b] : 1)        one IEEE fp32 division
 *   code      = #{ j : (NF4[j] + NF4[j+1]) / 2 < q }       a tie goes to the lower code
 *   packed[i] = code[2i] << 4 | code[2i+1]                 an odd numel is padded with a 0 (code 7)
 * Writes packed uint8[ceil(numel/2)] and absmax fp32[ceil(numel/blocksize)], nothing else.
 * blocksize: a power of two, 64..4096.  blocksize 64 with `w` 16-byte aligned and `packed`
 * 4-byte aligned takes the streaming kernel (one pass over the weight); every other
 * alignment (down to the element's own) and block size takes a slower general kernel.
 * NF4DQ_ERR_ARG: null pointer, bad dtype, unsupported blocksize, negative numel, `w` not
 * aligned to its element or `absmax` not to 4 bytes.  numel == 0: NF4DQ_OK, nothing launched. */
int nf4_quant_bnb(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize,
                  void* packed, void* absmax, void* hip_stream);

/* compress_statistics=True: the fp32 absmax goes to the workspace and is quantized in turn
 * with the 256-entry code book `code2` (device pointer, ascending; bitsandbytes' dynamic map):
 *   offset      = fp32( (sum of absmax, accumulated in fp64 in a fixed order) / nblk )
 *   v[i]        = absmax[i] - offset                       fp32; elements past nblk read as 0
 *   absmax2[g]  = max(max |v| over 256-block g, FLT_MIN)
 *   absmax_q[i] = #{ j : (code2[j] + code2[j+1]) / 2 < v[i] / absmax2[i / 256] }
 * Writes packed, absmax_q uint8[nblk], absmax2 fp32[ceil(nblk/256)], offset fp32[1] (on the
 * device) and the workspace.  Three launches on `hip_stream`, no host synchronisation, no
 * allocation, no float atomics (two runs give the same bits); capturable in a graph.
 * `offset` is the correctly rounded fp64 mean; the Python quantizer's fp32 reduction may
 * differ from it in the last bit, and absmax_q / absmax2 follow from the offset used.
 * blocksize2 must be 256.  `workspace`: 8-byte aligned, nf4_quant_workspace_bytes(numel,
 * blocksize) bytes, no initial contents required; a smaller one is NF4DQ_ERR_ARG. */
size_t nf4_quant_workspace_bytes(int64_t numel, int32_t blocksize);
int nf4_quant_bnb_nested(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize,
                         const float* code2, int32_t blocksize2,
                         void* packed, void* absmax_q, void* absmax2, void* offset,
                         void* workspace, size_t workspace_bytes, void* hip_stream);

/* Host forms: HOST pointers, synchronous, `threads` workers over the blocks (<= 0 = all
 * hardware threads), no workspace; the same results bit for bit, the same error codes. */
int nf4_quant_bnb_cpu(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize,
                      void* packed, void* absmax, int32_t threads);
int nf4_quant_bnb_nested_cpu(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize,
                             const float* code2, int32_t blocksize2,
                             void* packed, void* absmax_q, void* absmax2, void* offset,
                             int32_t threads);

/* Launch tuning (bench/tuning only; the entry points above use the default
 * {4, 0, 1, 0}).  tile_dwords must be 4 and nontemporal 1 (the tile shape and
 * the sc1+nt output stores every entry point uses; the other shapes and store
 * policies measured slower and were removed, profiles/r01/tune_sweep.log,
 * profiles/r02/x4_direct/).  blocks_per_cu: grid cap per CU (0 = one wave per
 * tile, no cap; capped grids walk tiles persistently).  flags: 0, or one of
 * NF4DQ_CFG_CHUNKS (the matrix goes through the path of every shape the flat
 * kernel does not take -- n % 64 != 0, padded rows, unaligned pointers: the chunk
 * kernels and, since round 6, the piece kernels -- even when it is flat-eligible) or
 * NF4DQ_CFG_ROWS (through the one-thread-per-byte general kernel, which otherwise
 * runs only past the chunk kernel's 32-bit index limits); for tests and tuning.
 * Other bits: NF4DQ_ERR_ARG.
 * (Absmax-line and page-translation prefetches were tried as flags and measured
 * no better than 1 %, profiles/r03/c5/; removed.) */
#define NF4DQ_CFG_ROWS 1
#define NF4DQ_CFG_CHUNKS 2
typedef struct nf4_launch_cfg {
    int32_t tile_dwords;
    int32_t blocks_per_cu;
    int32_t nontemporal;
    int32_t flags;
} nf4_launch_cfg;

int nf4_dequant_ref_cfg(const uint8_t* packed, int64_t packed_len,
                        const uint8_t* absmax_q, int64_t nb,
                        const float* absmax2, int64_t n2,
                        void* out, int32_t out_dtype, int64_t m, int64_t n,
                        const nf4_launch_cfg* cfg, void* hip_stream);

/* Fused dequant + GEMM for small M (decode-shaped activations; replaces the
 * reference harness's `X @ triton_dequantize_nf4(W).t()`, benchmark.py:61-66):
 *   y[M][N] = x[M][K] . W[N][K]^T,  W = the weights nf4_dequant_ref would
 *   write (reference semantics, bit-identical), fp32 accumulation (MFMA).
 * x, y: fp16/bf16 (out_dtype), row-major.  Fast-path shape rules (else
 * NF4DQ_ERR_SHAPE): M <= NF4DQ_GEMM_MAX_M, N % 64 == 0, K % 128 == 0,
 * packed_len == N*K/2 (and N <= 2^18).  `workspace` (16-byte aligned) must hold
 * nf4_gemm_workspace_bytes(M, N, K) bytes (0 = none needed): split-K ticket
 * counters + 64-bit partial-sum entries, handed between workgroups with relaxed
 * agent-scope atomics only and reduced inside the launch in a fixed order
 * (bitwise reproducible).  The workspace must be ZERO-FILLED before its first
 * use; every call leaves it reusable (counters and entries back to 0).  One
 * workspace per stream: concurrent calls must not share one. */
#define NF4DQ_GEMM_MAX_M 32
size_t nf4_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int nf4_gemm_ref(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                 const uint8_t* absmax_q, int64_t nb, const float* absmax2, int64_t n2,
                 void* y, int32_t out_dtype, int64_t N, int64_t K,
                 void* workspace, size_t workspace_bytes, void* hip_stream);

/* Tuning form of nf4_gemm_ref.  kernel: 0 = library choice,
 * NF4DQ_GEMM_STREAM (K % 256 == 0; waves 4/8/16, depth = chunks in flight per
 * wave 2/4/8 (8 not with 16 waves; 16 waves only when M <= 16), strips = 16-column strips per workgroup
 * 1/2/4 dividing waves) or NF4DQ_GEMM_K128 (waves 4/8, depth 1/2/4 (<= 2 when
 * M > 16), strips = 16-column strips per wave 1/2/4 (0 = 1), sharing x loads).  ksplit: K slices reduced across workgroups.
 * NF4DQ_GEMM_PERSIST: the streaming kernel's persistent form (M <= 16,
 * ksplit 1..16 K slices dividing K / 256, waves / strips K parts dividing a slice into a multiple of depth
 * (2/4), x[M][K] in LDS, absmax not wrapping inside a row).
 * An invalid combination returns NF4DQ_ERR_ARG. */
#define NF4DQ_GEMM_K128 1
#define NF4DQ_GEMM_STREAM 2
#define NF4DQ_GEMM_PERSIST 3
/* NF4DQ_GEMM_XS: shared-activation kernel (any M <= 32, K % 128 == 0): a
 * workgroup of `waves` (4/8) waves owns one 16-column strip per wave over a K
 * slice of `depth` (2/4/8) 128-deep chunks, the x slice staged once in LDS and
 * every weight chunk in flight at once; ksplit must equal ceil(K/128 / depth);
 * strips 0 or 1. */
#define NF4DQ_GEMM_XS 4
/* NF4DQ_GEMM_XR: register-resident activation kernel (any M <= 32, K % 128 ==
 * 0): the K split is over the `waves` (8/16) waves of a workgroup, each holding
 * its x fragments of `strips` 128-deep chunks in registers for the whole
 * launch; a workgroup walks its column strips with a `depth` (2/4) deep ring of
 * weight loads and sums the waves' partial tiles in LDS; `strips` = 128-deep
 * chunks per wave: 1, 2 (one 256-deep chunk, K % 256 == 0) or 4 (two, 8 waves
 * only, K % 512 == 0); ksplit must equal ceil(K/128 / (waves * strips))
 * (1 = no cross-workgroup reduction). */
#define NF4DQ_GEMM_XR 5
/* NF4DQ_GEMM_SK (6): retired in round 6.  The balanced ("stream-K") kernel was
 * never the library's choice (slower than the persistent kernel at every measured
 * shape) and no longer ships; a cfg naming it is rejected with NF4DQ_ERR_ARG. */
#define NF4DQ_GEMM_SK 6
/* NF4DQ_GEMM_GEMV: the decode GEMV (M == 1, K % 2048 == 0, K <= 16384, absmax not
 * wrapping inside a row): no MFMA; a lane dots 32 consecutive exact weights of a row
 * with x on the VALU.  waves 8/16 per workgroup, depth = rows per row group 1/2/4,
 * ksplit 1, strips = workgroups per CU 0/1/2 (0 = 1).  The library's choice at M = 1
 * for launches of up to 4096 columns. */
#define NF4DQ_GEMM_GEMV 7
typedef struct nf4_gemm_cfg {
    int32_t kernel;
    int32_t waves;
    int32_t depth;
    int32_t ksplit;
    int32_t strips;
} nf4_gemm_cfg;
size_t nf4_gemm_workspace_bytes_cfg(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg);
int nf4_gemm_ref_cfg(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                     const uint8_t* absmax_q, int64_t nb, const float* absmax2, int64_t n2,
                     void* y, int32_t out_dtype, int64_t N, int64_t K,
                     void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);

/* Several weights that share the activation x (q/k/v, gate/up): one launch.
 * Each weight: packed [N*K/2], its own absmax_q / absmax2 (reference wrap
 * semantics per weight), output y [M][N] (out_dtype).  Same shape rules as
 * nf4_gemm_ref for every weight (N % 64 == 0), at most NF4DQ_GEMM_GROUP_MAX
 * weights; cfg NULL = library choice for the summed N.  Every kernel runs
 * the group as one launch (the library's persistent choice falls back to one
 * launch per weight when absmax wraps inside a row).  Workspace as for
 * nf4_gemm_ref, sized by nf4_gemm_grouped_workspace_bytes. */
#define NF4DQ_GEMM_GROUP_MAX 8
typedef struct nf4_gemm_mat {
    const uint8_t* packed;
    int64_t packed_len;
    const uint8_t* absmax_q;
    int64_t nb;
    const float* absmax2;
    int64_t n2;
    void* y;
    int64_t N;
} nf4_gemm_mat;
size_t nf4_gemm_grouped_workspace_bytes(int64_t M, int64_t K, const nf4_gemm_mat* mats, int32_t count,
                                        const nf4_gemm_cfg* cfg);
int nf4_gemm_ref_grouped(const void* x, int64_t M, int64_t K, const nf4_gemm_mat* mats, int32_t count,
                         int32_t out_dtype, void* workspace, size_t workspace_bytes,
                         const nf4_gemm_cfg* cfg, void* hip_stream);

/* The fused GEMM in bitsandbytes semantics: y = x . W^T for the weight nf4_quant_bnb* /
 * bitsandbytes produce, a flat stream of N*K codes (row-major [N][K]) with one statistics
 * block per `blocksize` elements.  Element (r, c) lies in 64-block f = r * (K / 64) + c / 64
 * and statistics block i = f >> log2(blocksize / 64); its scale is
 *   nf4_gemm_bnb:         s = fl32(fl32(code2[absmax_q[i]] * absmax2[i / blocksize2]) + offset)
 *                         (two fp32 roundings, never a fused multiply-add)
 *   nf4_gemm_bnb_single:  s = absmax[i]
 * and W[r][c] = RNE16(fl32(NF4[code(r, c)] * s)), high nibble = even column: exactly the
 * values nf4_dequant_bnb / nf4_dequant_bnb_single write, bit for bit; fp32 accumulation and
 * one final rounding to out_dtype (fp16 / bf16).  Statistics never wrap around in this mode.
 * `code2`: 256 fp32 on the device.  `offset`: ONE fp32 ON THE DEVICE, read by the kernel
 * (no host copy, no synchronisation; it may change between calls); NULL = 0.
 * Shape rules as nf4_gemm_ref (M <= NF4DQ_GEMM_MAX_M, N % 64 == 0, K % 128 == 0, packed_len
 * == N*K/2; else NF4DQ_ERR_SHAPE).  blocksize: a power of two, 64..4096; blocksize2: a power
 * of two >= 4 (else NF4DQ_ERR_ARG).  nb / nabs >= ceil(N*K / blocksize) and n2 >= ceil(that /
 * blocksize2), else NF4DQ_ERR_SHAPE.  A null code2 / absmax2 / absmax_q: NF4DQ_ERR_ARG.
 * M == 0 or N == 0: NF4DQ_OK, nothing launched.
 * cfg NULL = the library's choice: what nf4_gemm_ref runs for (M, N, K) -- same kernel, same
 * decomposition -- where that kernel has the mode, else the 128-deep kernel.  A cfg may
 * name NF4DQ_GEMM_K128, _PERSIST, _XR or _GEMV (their rules above); with blocksize > 64
 * only NF4DQ_GEMM_K128.  NF4DQ_GEMM_STREAM and NF4DQ_GEMM_XS do not have the mode:
 * NF4DQ_ERR_ARG, as for any invalid cfg.
 * Workspace (nf4_gemm_bnb_workspace_bytes; with cfg NULL enough for any blocksize), its
 * zero-fill contract, the split-K error word and nf4_gemm_check_workspace: exactly as for
 * nf4_gemm_ref.  Asynchronous on `hip_stream`; allocates nothing. */
size_t nf4_gemm_bnb_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                 const uint8_t* absmax_q, int64_t nb, const float* code2,
                 const float* absmax2, int64_t n2, const float* offset,
                 int32_t blocksize, int32_t blocksize2,
                 void* y, int32_t out_dtype, int64_t N, int64_t K,
                 void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);
int nf4_gemm_bnb_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                        const float* absmax, int64_t nabs, int32_t blocksize,
                        void* y, int32_t out_dtype, int64_t N, int64_t K,
                        void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);

/* Several weights in bitsandbytes semantics that share the activation x (q/k/v, gate/up):
 * one launch.  `mats` points at `count` nf4_gemm_bnb_mat (it is `const void*` so that every
 * prototype of this header keeps to the plain parameter types bindings are derived from).
 * Every weight has its own code2 table, offset pointer, blocksize and blocksize2, and its
 * statistics are indexed on its own flat stream (64-block f = row_in_weight * (K / 64) +
 * block, from 0 for each weight); the values are nf4_gemm_bnb's / nf4_gemm_bnb_single's per
 * weight, bit for bit in the weights entering the products.  All weights of a call are
 * nested (single == 0) or all have fp32 statistics (single != 0: absmax_q, code2, offset
 * and blocksize2 are ignored; absmax2 / n2 are the fp32 absmax and its length).
 * Rules: nf4_gemm_bnb's per weight (block sizes, null fields: NF4DQ_ERR_ARG; N % 64,
 * packed_len, statistics lengths: NF4DQ_ERR_SHAPE) and nf4_gemm_ref_grouped's for the group
 * (count <= NF4DQ_GEMM_GROUP_MAX, K % 128 == 0, M <= NF4DQ_GEMM_MAX_M; an N == 0 weight is
 * accepted by the families that number column groups per weight -- K128 and XR -- and is
 * NF4DQ_ERR_SHAPE under the persistent kernel).  count == 0, M == 0 or no columns at all:
 * NF4DQ_OK, nothing launched.
 * cfg NULL = the library's choice: one launch -- what nf4_gemm_ref_grouped runs for the
 * column total where that family has the grouped mode and every blocksize is 64, the
 * persistent kernel where that would be the decode GEMV, else the 128-deep kernel; only a
 * persistent choice that cannot run falls back to one nf4_gemm_bnb launch per weight.  A cfg
 * may name NF4DQ_GEMM_K128, _PERSIST or _XR; any other family, or any but K128 when a weight
 * has blocksize > 64, is NF4DQ_ERR_ARG, and a named cfg never falls back.  The decode GEMV,
 * the streaming and the shared-activation kernels do not have the grouped mode.  A call with
 * one weight runs as nf4_gemm_bnb / nf4_gemm_bnb_single does.
 * Workspace (nf4_gemm_bnb_grouped_workspace_bytes), its zero-fill contract, the split-K
 * error word and nf4_gemm_check_workspace: exactly as for nf4_gemm_ref_grouped.
 * Asynchronous on `hip_stream`; allocates nothing. */
typedef struct nf4_gemm_bnb_mat {
    const uint8_t* packed;
    int64_t packed_len;      /* N*K/2 */
    const uint8_t* absmax_q; /* nested; NULL in single mode */
    int64_t nb;              /* nested; 0 in single mode */
    const float* code2;      /* nested: 256 fp32 on the device; NULL in single mode */
    const float* absmax2;    /* nested: absmax2; single: the fp32 absmax */
    int64_t n2;              /* ... and its length */
    const float* offset;     /* nested: ONE fp32 on the device, or NULL (= 0) */
    int32_t blocksize, blocksize2; /* per weight; blocksize2 ignored in single mode */
    void* y;
    int64_t N;
} nf4_gemm_bnb_mat;
size_t nf4_gemm_bnb_grouped_workspace_bytes(int64_t M, int64_t K, const void* mats, int32_t count,
                                            int32_t single, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_grouped(const void* x, int64_t M, int64_t K, const void* mats, int32_t count,
                         int32_t single, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                         const nf4_gemm_cfg* cfg, void* hip_stream);

/* The fused GEMM in bitsandbytes semantics for 33..128 rows (batched decode, a speculative
 * verify step, a short prompt): the row-tiled kernel family.  The values are nf4_gemm_bnb's /
 * nf4_gemm_bnb_single's: W bit for bit what nf4_dequant_bnb / nf4_dequant_bnb_single write (two
 * fp32 products and one RNE per weight, never a fused multiply-add; `offset` ONE fp32 ON THE
 * DEVICE, NULL = 0), fp32 accumulation on MFMA, one final rounding to out_dtype (fp16 / bf16).
 * Every weight is decoded once per workgroup and multiplied with all row tiles; x is staged
 * through LDS in 128-deep chunks.
 * Shapes: 1 <= M <= NF4DQ_GEMM_MT_MAX_M (the whole range, so that tile edges can be tested;
 * below 33 rows nf4_gemm_bnb is the faster entry), N % 64 == 0 and N >= 64, K % 128 == 0 and
 * K >= 128, packed_len == N*K/2, blocksize == 64 (a larger valid blocksize: NF4DQ_ERR_SHAPE),
 * nb / nabs >= N*K/64 and n2 >= ceil(that / blocksize2); else NF4DQ_ERR_SHAPE -- M == 0 and
 * N == 0 included.  N > 2^18: NF4DQ_ERR_TOO_LARGE.  A null pointer (offset excepted), x / packed
 * not 16-byte or y not 8-byte aligned, a bad dtype or a block size that is no power of two:
 * NF4DQ_ERR_ARG.
 * cfg NULL = the library's choice.  A cfg names kernel NF4DQ_GEMM_MT (0 = the same) with
 *   waves   waves per workgroup, 2 / 4: a workgroup owns 32 * waves columns (N must divide)
 *   depth   K stage in 128-deep chunks: 1
 *   ksplit  K slices, 1 .. min(K / 128, 16); ceil(K/128 / ksplit) chunks per slice, so the
 *           last slices may be short or empty
 *   strips  16-column strips per wave: 2 (0 = 2)
 * and never falls back: an invalid one is NF4DQ_ERR_ARG.  The row-tile count follows from M.
 * Workspace (nf4_gemm_bnb_mt_workspace_bytes; 0 = none, one K slice): nf4_gemm_ref's layout
 * and contract -- 16-byte aligned, zero-filled before its first use, left zero by every call,
 * one per stream, shareable with the other fused entries.  K slices write fp32 partials to a
 * slab, make them visible (agent-scope release) and draw a ticket; the slice drawing the last
 * ticket acquires, sums all slices in slice order, stores y and clears the slab and the
 * ticket.  No workgroup waits for another, so this family cannot time out and never sets the
 * split-K error word; the result is a function of the inputs and the cfg alone.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_GEMM_MT_MAX_M 128
#define NF4DQ_GEMM_MT 8
size_t nf4_gemm_bnb_mt_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_mt(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                    const uint8_t* absmax_q, int64_t nb, const float* code2,
                    const float* absmax2, int64_t n2, const float* offset,
                    int32_t blocksize, int32_t blocksize2,
                    void* y, int32_t out_dtype, int64_t N, int64_t K,
                    void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);
int nf4_gemm_bnb_mt_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                           const float* absmax, int64_t nabs, int32_t blocksize,
                           void* y, int32_t out_dtype, int64_t N, int64_t K,
                           void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);

/* The fused expert GEMM of a mixture-of-experts block in bitsandbytes semantics: ONE launch
 * per projection for all experts, routed on the device.  With `experts` weights of one shape
 * [N][K], P (token, choice) pairs and int32 expert_ids[P] ON THE DEVICE,
 *   y[p][:] = x[p / x_div][:] . W_{expert_ids[p]}^T          for p in 0 .. P-1
 * with W_e bit for bit what nf4_dequant_bnb / nf4_dequant_bnb_single write for expert e (nested:
 * fl32(fl32(code2_e[absmax_q] * absmax2) + offset_e), then the code times that scale with one
 * RNE to 16 bits, never a fused multiply-add), fp32 accumulation on MFMA and one final rounding
 * to out_dtype (fp16 / bf16).  x_div = how many consecutive pairs share one row of x: top_k for
 * a projection of the token's hidden state (x has ceil(P / x_div) rows; nothing past them is
 * read), 1 for one of per-pair activations.  A pair whose id is outside [0, experts) gets a row
 * of zeros, as nf4_embedding_bnb treats an id outside the table; one token may name the same
 * expert twice.  Every row of y ([P][N], dense) is stored by the launch; nothing else is
 * written but the workspace.  The ids are read when the kernel runs: no host copy, no
 * synchronisation, and a captured graph follows the router from replay to replay.  An expert
 * without a pair costs no weight or statistics traffic.
 * The experts are stacked: one base pointer per kind of data and a stride between experts
 * (`experts` points at ONE nf4_moe_experts in host memory; it is `const void*`, as `expert_ids`
 * is, so that every prototype of this header keeps to the plain parameter types bindings are
 * derived from).  Every expert has its own statistics, its own offset and, with code2_stride
 * != 0, its own code2 table.
 * Rules (nf4_gemm_bnb_mt's, with its codes): 1 <= P <= NF4DQ_MOE_MAX_PAIRS, N % 64 == 0 and
 * N >= 64, K % 128 == 0 and K >= 128, blocksize == 64 (a larger valid one: NF4DQ_ERR_SHAPE),
 * packed_stride >= N*K/2, nb_stride >= N*K/64, n2_stride >= ceil(N*K/64 / blocksize2) (single:
 * >= N*K/64), code2_stride 0 or >= 256; else NF4DQ_ERR_SHAPE.  N > 2^18, more split-K tickets
 * (experts * column tiles) than the workspace header holds: NF4DQ_ERR_TOO_LARGE.  A null
 * pointer (offset excepted), x / packed not 16-byte, y not 8-byte or expert_ids not 4-byte
 * aligned, packed_stride % 16 != 0, a bad dtype, a block size that is no power of two,
 * experts outside 1 .. NF4DQ_MOE_MAX_EXPERTS, x_div < 1 or a negative size: NF4DQ_ERR_ARG.
 * P == 0: NF4DQ_OK, nothing launched.
 * cfg NULL = the library's choice from (P, experts, N, K, CU count) alone.  A cfg names kernel
 * NF4DQ_GEMM_MOE (0 = the same) with nf4_gemm_bnb_mt's fields (waves 2 / 4, depth 1, ksplit
 * 1 .. min(K / 128, 16), strips 2 or 0) and never falls back: an invalid one is NF4DQ_ERR_ARG.
 * Workspace (nf4_gemm_bnb_moe_workspace_bytes; 0 = none, one K slice): nf4_gemm_ref's layout and
 * contract -- the ticket header, then ksplit slabs of P * N floats indexed by pair, all zero
 * between calls, shareable with the other fused entries.  One ticket per (expert, column
 * tile); no workgroup waits for another, so the split-K error word is never set, and the result
 * is a function of the inputs and the cfg alone.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_MOE_MAX_PAIRS 128
#define NF4DQ_MOE_MAX_EXPERTS 256
#define NF4DQ_GEMM_MOE 9
typedef struct nf4_moe_experts {
    const uint8_t* packed;   /* expert e: packed + e * packed_stride, N*K/2 bytes */
    int64_t packed_stride;   /* bytes between experts, >= N*K/2, % 16 == 0 */
    const uint8_t* absmax_q; /* nested; NULL in single mode */
    int64_t nb_stride;       /* bytes between experts; 0 in single mode */
    const float* code2;      /* nested: 256 fp32 on the device per table; NULL in single mode */
    int64_t code2_stride;    /* floats: 0 = one table shared by all experts, else >= 256 */
    const float* absmax2;    /* nested: absmax2; single: the fp32 absmax */
    int64_t n2_stride;       /* floats between experts */
    const float* offset;     /* nested: `experts` fp32 ON THE DEVICE, or NULL (= 0) */
    int64_t N, K;            /* every expert's shape */
    int32_t experts;         /* 1 .. NF4DQ_MOE_MAX_EXPERTS */
    int32_t single;          /* 0: nested statistics; != 0: fp32 absmax */
    int32_t blocksize, blocksize2; /* blocksize2 ignored in single mode */
} nf4_moe_experts;
size_t nf4_gemm_bnb_moe_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_moe(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts,
                     void* y, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                     const nf4_gemm_cfg* cfg, void* hip_stream);

/* nf4_gemm_bnb_moe beyond 128 pairs: the same product, descriptor, rules, alignments, order of
 * status codes and workspace contract for 1 <= P <= NF4DQ_MOE_RB_MAX_PAIRS (token, choice) pairs
 * in ONE launch -- a decode batch of 32 sequences at top-8, a speculative verify step, a short
 * prompt.  The ids are still read on the device only, so the call is capturable and a replay
 * follows the router.  The grid is experts x column tiles x K slices x ceil(P / 128) row blocks,
 * fixed by the host whatever the routing: a workgroup lists its expert's pairs in ascending order
 * by ballots over all P ids and owns entries [128 rb, 128 rb + 128) of that list; one whose
 * expert has no more than 128 rb pairs returns before any weight or statistics load.  An expert's
 * weight is therefore read once per row block it fills, an idle expert's never.  A row's fp32 sum
 * depends on the chunk order and the K slices alone, so every row's bits are those
 * nf4_gemm_bnb_moe stores for that row at the cfg with the same waves and ksplit, and for
 * P <= 128 the two entries' outputs are equal bit for bit.
 * P > NF4DQ_MOE_RB_MAX_PAIRS: NF4DQ_ERR_SHAPE; P == 0: NF4DQ_OK, nothing launched.  More split-K
 * tickets (experts * column tiles * row blocks) than the workspace header holds, or K slices
 * whose slab (ksplit * P * N floats) reaches 2^32 bytes: NF4DQ_ERR_TOO_LARGE.
 * cfg NULL = the library's choice from (P, experts, N, K, CU count) alone.  A cfg names kernel
 * NF4DQ_GEMM_MOE_RB (0 = the same) with nf4_gemm_bnb_moe's fields and never falls back: an invalid
 * one, NF4DQ_GEMM_MOE included, is NF4DQ_ERR_ARG.
 * Workspace (nf4_gemm_bnb_moe_rb_workspace_bytes; 0 = none, one K slice): nf4_gemm_bnb_moe's
 * layout and contract -- the ticket header, then ksplit slabs of P * N floats indexed by pair, all
 * zero between calls, shareable with the other fused entries on the same stream.  One ticket per
 * (expert, column tile, row block); no workgroup waits for another.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_MOE_RB_MAX_PAIRS 1024
#define NF4DQ_GEMM_MOE_RB 13
size_t nf4_gemm_bnb_moe_rb_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_moe_rb(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts,
                        void* y, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                        const nf4_gemm_cfg* cfg, void* hip_stream);

/* The first half of a Llama-family MLP, `silu(gate(x)) * up(x)`, in bitsandbytes semantics for
 * 1..128 rows: ONE launch of the row-tiled family over the gate and the up weight, which share
 * x and the shape [I][K].  With dt = out_dtype (fp16 / bf16) and rn = round-to-nearest-even to dt,
 *   g = rn(x . Wg^T)   u = rn(x . Wu^T)      exactly what nf4_gemm_bnb_mt stores for each weight
 *   s = rn(g / (1.0f + expf(-g)))             fp32, IEEE division, never a fused multiply-add
 *   h = rn(s * u)                             the fp32 product of two 16-bit values is exact
 * -- the rounding chain of `F.silu(gate(x)) * up(x)` on 16-bit tensors; Wg / Wu bit for bit what
 * nf4_dequant_bnb / nf4_dequant_bnb_single write.  A non-finite g or u gives whatever the chain
 * gives.  A wave owns 16 columns of h: its two strips are the same 16 rows of the gate and of
 * the up weight, so g and u of an element meet in one lane and neither makes a trip through
 * memory.
 * `gate_up` points at TWO nf4_gemm_bnb_mat in host memory, the gate weight then the up weight
 * (`const void*`, as in nf4_gemm_bnb_grouped); they are not interchangeable.  Each has its own
 * statistics, code2 table, offset (ONE fp32 ON THE DEVICE, NULL = 0) and blocksize2; both are
 * nested (single == 0) or both have fp32 statistics (single != 0: absmax_q, code2, offset and
 * blocksize2 are ignored).  Both N fields must equal I; the y fields are ignored.  `act` names
 * the activation: NF4DQ_ACT_SILU (any other: NF4DQ_ERR_ARG).  h is [M][I], dense.
 * Rules: nf4_gemm_bnb_mt's, per weight -- 1 <= M <= NF4DQ_GEMM_MT_MAX_M, I % 64 == 0 and
 * I >= 64, K % 128 == 0 and K >= 128, the two N equal, packed_len == I*K/2, blocksize == 64 (a
 * larger valid one: NF4DQ_ERR_SHAPE), nb / n2 as there; else NF4DQ_ERR_SHAPE.  I > 2^18 and the
 * other size limits of nf4_gemm_bnb_mt: NF4DQ_ERR_TOO_LARGE.  A null pointer (offset excepted),
 * x / packed not 16-byte or h not 8-byte aligned, a bad dtype, a block size that is no power of
 * two: NF4DQ_ERR_ARG.
 * cfg NULL = the library's choice.  A cfg names kernel NF4DQ_GEMM_MT_SWIGLU (0 = the same) with
 *   waves   waves per workgroup, 2 / 4: a workgroup owns 16 * waves columns of h
 *   depth   K stage in 128-deep chunks: 1
 *   ksplit  K slices, 1 .. min(K / 128, 16); the last slices may be short or empty
 *   strips  16-row weight strips per wave: 2 (one of gate, one of up; 0 = 2)
 * and never falls back: an invalid one is NF4DQ_ERR_ARG.
 * Workspace (nf4_gemm_bnb_mt_swiglu_workspace_bytes; 0 = none, one K slice): nf4_gemm_bnb_mt's
 * layout and contract -- the ticket header, then per K slice the gate plane and the up plane of
 * M * I floats ([ksplit][2][M][I]); 16-byte aligned, zero-filled before its first use, left zero
 * by every call, one per stream, shareable with the other fused entries.  One ticket per column
 * tile; the slice drawing the last one sums each plane in slice order, applies the chain, stores
 * h and clears the planes and the ticket.  No workgroup waits for another, so the split-K error
 * word is never set, and the result is a function of the inputs and the cfg alone.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_GEMM_MT_SWIGLU 10
#define NF4DQ_ACT_SILU 0
size_t nf4_gemm_bnb_mt_swiglu_workspace_bytes(int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_mt_swiglu(const void* x, int64_t M, int64_t K,
                           const void* gate_up /* nf4_gemm_bnb_mat[2]: gate, up */, int32_t single,
                           int32_t act, void* h, int32_t out_dtype,
                           void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);

/* The first half of a mixture-of-experts block, `silu(w1(x)) * w3(x)` per (token, choice) pair,
 * in bitsandbytes semantics: ONE launch for all experts, routed on the device -- the expert
 * GEMM's anatomy (nf4_gemm_bnb_moe) with the SwiGLU launch's two-weight strips and rounding
 * chain (nf4_gemm_bnb_mt_swiglu).  With int32 expert_ids[P] ON THE DEVICE, e = expert_ids[p] and
 * rn = round-to-nearest-even to out_dtype (fp16 / bf16), for p in 0 .. P-1
 *   g = rn(x[p / x_div] . Wg_e^T)   u = rn(x[p / x_div] . Wu_e^T)   what nf4_gemm_bnb_moe stores
 *                                                                   for each stack
 *   s = rn(g / (1.0f + expf(-g)))   h[p] = rn(s * u)                nf4_gemm_bnb_mt_swiglu's chain
 * A pair whose id is outside [0, experts) gets a row of zero bits.  Every row of h ([P][I],
 * dense) is stored by the launch; nothing else is written but the workspace.  The ids and the
 * offsets are read when the kernel runs: no host copy, no synchronisation.  An expert without a
 * pair costs no weight or statistics traffic.  Neither g nor u makes a trip through memory.
 * `gate_up` points at TWO nf4_moe_experts in host memory, the gate stack (Mixtral's w1) then the
 * up stack (w3); they are not interchangeable.  Each stack has its own base pointers, strides,
 * statistics, offsets, code2 tables (code2_stride 0 = one table for its experts) and blocksize2;
 * the two must agree in N (= I), K, experts and single (else NF4DQ_ERR_SHAPE).  `act` names the
 * activation: NF4DQ_ACT_SILU (any other: NF4DQ_ERR_ARG).
 * Rules: nf4_gemm_bnb_moe's with its codes and order, per stack -- 1 <= P <= NF4DQ_MOE_MAX_PAIRS,
 * I % 64 == 0 and I >= 64, K % 128 == 0 and K >= 128, blocksize == 64, the strides long enough;
 * else NF4DQ_ERR_SHAPE.  I > 2^18, more split-K tickets (experts * column tiles) than the
 * workspace header holds, a workspace need of 2^32 bytes or more: NF4DQ_ERR_TOO_LARGE.  A null
 * pointer (offset excepted), x / packed not 16-byte, h not 8-byte or expert_ids not 4-byte
 * aligned, packed_stride % 16 != 0, a bad dtype, a block size that is no power of two, experts
 * outside 1 .. NF4DQ_MOE_MAX_EXPERTS, x_div < 1 or a negative size: NF4DQ_ERR_ARG.  P == 0:
 * NF4DQ_OK, nothing launched.
 * cfg NULL = the library's choice from (P, experts, I, K, CU count) alone.  A cfg names kernel
 * NF4DQ_GEMM_MOE_SWIGLU (0 = the same) with nf4_gemm_bnb_mt_swiglu's fields (waves 2 / 4: a
 * workgroup owns 16 * waves columns of h; depth 1; ksplit 1 .. min(K / 128, 16); strips 2 or 0)
 * and never falls back: an invalid one is NF4DQ_ERR_ARG.
 * Workspace (nf4_gemm_bnb_moe_swiglu_workspace_bytes; 0 = none, one K slice): the ticket header,
 * then per K slice the gate plane and the up plane of P * I floats indexed by pair
 * ([ksplit][2][P][I]), all zero between calls, shareable with the other fused entries.  One
 * ticket per (expert, column tile); the slice drawing the last one sums each plane in slice
 * order over the expert's rows and applies the chain.  No workgroup waits for another, so the
 * split-K error word is never set, and the result is a function of the inputs and the cfg alone.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_GEMM_MOE_SWIGLU 11
size_t nf4_gemm_bnb_moe_swiglu_workspace_bytes(int64_t P, const void* gate_up, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_moe_swiglu(const void* x, const void* expert_ids, int64_t P, int32_t x_div,
                            const void* gate_up /* nf4_moe_experts[2]: gate, up */, int32_t act,
                            void* h, int32_t out_dtype,
                            void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);

/* The second half of a mixture-of-experts block, the down projection (Mixtral's w2) WITH the
 * routed weighted sum, in bitsandbytes semantics: ONE launch for all experts, routed on the
 * device -- the expert GEMM (nf4_gemm_bnb_moe) with the combine of a token's `topk` pairs behind
 * it.  With int32 expert_ids[P] and routing_weights[P] ON THE DEVICE, e = expert_ids[p] and
 * rn = round-to-nearest-even to out_dtype (fp16 / bf16), for t in 0 .. P / topk - 1
 *   d[p] = rn(x[p / x_div] . W_e^T)                   exactly what nf4_gemm_bnb_moe stores for the
 *                                                     pair under the same (waves, ksplit);
 *                                                     +0 for an id outside [0, experts)
 *   y[t] = rn(sum_j rn(d[t topk + j] * rn(rw[t topk + j])))     j = 0 .. topk-1
 * The product is formed in fp32 (exact for two 16-bit values) and rounded once; the sum is fp32,
 * starts from +0.0f and adds j = 0, 1, .. in that order, rounded once -- the rounding chain of
 * `(d * rw.to(dtype).unsqueeze(-1)).sum(dim=1)` on 16-bit tensors with the order spelled out, so
 * -0 + -0 gives +0 and a NaN weight gives NaN also for an invalid id.  y is [P / topk][N], dense;
 * every row is stored by the launch; the [P][N] products never leave the workspace.
 * `routing_weights` is fp32 (rw_dtype NF4DQ_F32: rounded to out_dtype on the device, as a cast
 * does) or out_dtype (rw_dtype == out_dtype); 4-byte or 2-byte aligned.  Any other rw_dtype,
 * topk < 1, topk > P or P % topk != 0: NF4DQ_ERR_ARG.
 * Every other rule, code and their order are nf4_gemm_bnb_moe's: 1 <= P <= NF4DQ_MOE_MAX_PAIRS,
 * N % 64 == 0, K % 128 == 0, blocksize == 64, the alignments (y 8-byte), the size limits.
 * P == 0: NF4DQ_OK, nothing launched.
 * cfg NULL = the library's choice, nf4_gemm_bnb_moe's for the same (P, experts, N, K, CU count).
 * A cfg names kernel NF4DQ_GEMM_MOE_DOWN (0 = the same) with nf4_gemm_bnb_moe's fields and never
 * falls back: an invalid one is NF4DQ_ERR_ARG.
 * Workspace (nf4_gemm_bnb_moe_down_workspace_bytes; never 0 for a valid call): the ticket header
 * -- experts * column tiles tickets of the K slices, then one ticket per column tile for the
 * combine; more than the header holds: NF4DQ_ERR_TOO_LARGE --, then ksplit slabs of P * N floats
 * when ksplit > 1, then P * N 16-bit products.  The workspace is zero before its first use and is
 * this entry's alone (another entry's slabs must be zero where this one leaves its products).  The
 * header is zero after every call.  The products are don't-care: every one read was written by the
 * same call.  The slabs are zero between calls of one (P, N, ksplit).  Where one workspace serves
 * calls of different (P, N, ksplit), an earlier call's products may lie where a later call has its
 * slabs: every slab element a reducer reads was stored by a slice of the same call, so the result
 * is the same, and afterwards the slab rows of pairs with a valid id are zero, while those of
 * pairs without one keep what lay there.
 * Per column tile each expert arrives once, after its rows are stored (an expert without
 * a pair at once, with no weight or statistics traffic); the last arrival combines the tile.  No
 * workgroup waits for another, so the split-K error word is never set, and the result is a
 * function of the inputs and the cfg alone.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_GEMM_MOE_DOWN 12
size_t nf4_gemm_bnb_moe_down_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg);
int nf4_gemm_bnb_moe_down(const void* x, const void* expert_ids, int64_t P, int32_t x_div, int32_t topk,
                          const void* routing_weights, int32_t rw_dtype, const void* experts, void* y,
                          int32_t out_dtype, void* workspace, size_t workspace_bytes,
                          const nf4_gemm_cfg* cfg, void* hip_stream);

/* The low-rank adapter tail of a Linear4bit (LoRA), one launch for up to NF4DQ_LORA_GROUP_MAX
 * adapters that share the activations x [M][K]:  y_i = base_i + scale_i * B_i (A_i x).
 * `mats` points at `count` nf4_lora_mat descriptors ON THE HOST (read during the call only).
 * With rn = round-to-nearest-even to `dtype` (fp16 / bf16: x, A [r][K], B [N][r], base [M][N] and
 * y [M][N] all have it, dense and row-major), per adapter
 *   t[m][j] = rn(sum_k x[m][k] * A[j][k])          fp32 accumulation
 *   u[m][n] = rn(sum_j t[m][j] * B[n][j])          fp32 accumulation
 *   v[m][n] = rn(float(u[m][n]) * scale)           one fp32 product, rounded once more
 *   y[m][n] = rn(float(base[m][n]) + float(v[m][n]))     base NULL: y = v
 * -- the rounding chain of `result + lora_B(lora_A(x)) * scaling` on 16-bit tensors.  The order of
 * the two sums is the kernel's: a function of (M, K, the r and N of the group, tile_n, waves)
 * alone -- no float atomics, the same bits on every call.  base == y (in place) is the normal use:
 * every output element is read and written once, by one lane.  Two adapters of one call must not
 * share output elements.
 * Domain: 1 <= M <= NF4DQ_LORA_MAX_M, K % 32 == 0, N % 16 == 0, r % 8 == 0 and
 * 8 <= r <= NF4DQ_LORA_MAX_R, 1 <= count <= NF4DQ_LORA_GROUP_MAX, every pointer 16-byte aligned.
 * Codes: a null x / mats / A / B / y, a dtype that is not fp16 or bf16, a count or an r outside
 * its limits, an invalid cfg: NF4DQ_ERR_ARG.  M, K, N or r % 8 outside the domain, a misaligned
 * pointer: NF4DQ_ERR_SHAPE.  K or N above 2^22: NF4DQ_ERR_TOO_LARGE.  Checked in that order.
 * cfg NULL = the library's choice for (M, K, the group's N and r, CU count); a nf4_lora_cfg names
 * tile_n in {16, 32, 64, 128, 256} and waves in {1, 2, 4} and never falls back.
 * The grid is (adapter, tile of tile_n columns); every workgroup forms its adapter's whole t in
 * LDS (K split over its waves, partials summed in wave order), then each wave takes 16-column
 * strips of the tile.  No workspace, no host read of device memory, no workgroup waits for
 * another.  Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph. */
#define NF4DQ_LORA_MAX_M 128
#define NF4DQ_LORA_MAX_R 128
#define NF4DQ_LORA_GROUP_MAX 8 /* = NF4DQ_GEMM_GROUP_MAX */
typedef struct {
    const void* A;    /* [r][K] */
    const void* B;    /* [N][r] */
    const void* base; /* [M][N], or NULL; may be y */
    void* y;          /* [M][N] */
    int64_t N;
    int32_t r;
    float scale;
} nf4_lora_mat;
typedef struct {
    int32_t tile_n; /* columns per workgroup */
    int32_t waves;  /* waves per workgroup */
} nf4_lora_cfg;
int nf4_lora_add(const void* x, int64_t M, int64_t K, const void* mats, int32_t count, int32_t dtype,
                 const void* cfg, void* hip_stream);

/* The adapter tail of a Linear4bit for a batch whose rows belong to DIFFERENT adapters (one NF4
 * base, many LoRA adapters), one launch for up to NF4DQ_LORA_GROUP_MAX stacks (q/k/v) that share
 * the activations x [M][K], the ids and the number of adapters S = `adapters`:
 *   a = adapter_ids[m]        int32 [M] ON THE DEVICE, read when the kernel runs
 *   0 <= a < S:  y_i[m] = base_i[m] + scale_i[a] * B_i[a] (A_i[a] x[m])
 *   otherwise (-1, S, INT32_MIN, ..): the row has no adapter; y_i[m] is base_i[m] bit for bit, a
 *                row of +0 with base NULL, and with base == y nothing is stored.
 * `stacks` points at `count` nf4_lora_stack descriptors ON THE HOST (read during the call only).
 * Adapter s of a stack is A + s * a_stride ([r][K]) and B + s * b_stride ([N][r]), strides in
 * elements; scale is fp32 [S] ON THE DEVICE; an adapter of a smaller rank is zero-padded to the
 * stack's r by the caller.  A row with an adapter gets nf4_lora_add's rounding chain exactly
 *   t = rn(sum_k x[m][k] A_a[j][k])   u = rn(sum_j t[j] B_a[n][j])   v = rn(float(u) * scale[a])
 *   y[m][n] = rn(float(base[m][n]) + float(v))                 base NULL: y = v
 * with fp32 accumulation, and its summation: the K / 32 chunks split into one contiguous range
 * per wave, summed in chunk order, the waves' partials in wave order, the expand over r in order.
 * So a row's bits are a function of x[m], its adapter, base[m], K, r and cfg.waves alone -- not of
 * M, the row's position or the other rows and ids of the batch -- and equal what nf4_lora_add
 * stores for that row with that adapter and the same waves; a zero-padded adapter gives the bits
 * of the unpadded one for every row of x that is finite.  A row of x that holds an infinity meets
 * the padding as inf * 0 = NaN in the padded columns of t, so its whole output row is NaN where the
 * unpadded adapter gives infinities: the chain above on the padded matrices, not a special case.
 * No float atomics, the same bits on every call.  base == y (in place) is
 * the normal use: every output element is read and written once, by one lane.  Two stacks of one
 * call must not share output elements.
 * Domain: nf4_lora_add's (M, K, N, r, count, 16-byte alignment of x, A, B, base, y), and
 * 1 <= adapters <= NF4DQ_LORA_MAX_ADAPTERS, ids and scale 4-byte aligned, a_stride and b_stride
 * multiples of 8 with a_stride >= r * K and b_stride >= N * r.
 * Codes: a null x / adapter_ids / stacks / A / B / scale / y, a dtype that is not fp16 or bf16, a
 * count, an `adapters` or an r outside its limits, an invalid cfg: NF4DQ_ERR_ARG.  M, K, N or
 * r % 8 outside the domain, a misaligned pointer, a stride that is no multiple of 8 or smaller
 * than one adapter: NF4DQ_ERR_SHAPE.  K or N above 2^22, a stride above 2^40:
 * NF4DQ_ERR_TOO_LARGE.  Checked in that order.
 * cfg NULL = the library's choice for (M, adapters, the stacks' N, CU count); a nf4_lora_cfg
 * names tile_n and waves as for nf4_lora_add and never falls back.
 * The grid is (stack, slot, tile of tile_n columns) with slot < min(adapters, M).  Every wave
 * reads the M ids and ballots; a workgroup takes the slot-th smallest adapter PRESENT, lists its
 * rows in LDS in ascending order, forms t for those rows only, expands its tile and scatters the
 * rows to y; a workgroup whose slot is beyond the adapters present returns before it loads a byte
 * of x, A or B, and slot 0's workgroups store the rows without an adapter when base != y.  No
 * workspace, no atomics, no host read of device memory, no workgroup waits for another.
 * Asynchronous on `hip_stream`; one launch; allocates nothing; capturable in a graph, and a
 * replay follows whatever ids the buffer then holds. */
#define NF4DQ_LORA_MAX_ADAPTERS 64
typedef struct {
    const void* A;      /* [S][r][K], adapter s at A + s * a_stride elements */
    const void* B;      /* [S][N][r], adapter s at B + s * b_stride elements */
    const float* scale; /* [S] fp32, ON THE DEVICE */
    const void* base;   /* [M][N], or NULL; may be y */
    void* y;            /* [M][N] */
    int64_t N;
    int64_t a_stride;
    int64_t b_stride;
    int32_t r;          /* the stack's rank; a smaller adapter is zero-padded by the caller */
} nf4_lora_stack;
int nf4_lora_add_routed(const void* x, const void* adapter_ids, int64_t M, int64_t K, int32_t adapters,
                        const void* stacks, int32_t count, int32_t dtype, const void* cfg, void* hip_stream);

/* The split-K hand-off never hangs: a reducer that has polled a partner slice's
 * entries 2^16 times without seeing them gives up, reads them as NaN and sets a
 * sticky error word in the workspace header.  This call waits for `hip_stream`,
 * reads that word and returns NF4DQ_OK, or NF4DQ_ERR_SPLITK_TIMEOUT after
 * zero-filling the whole workspace again (a stalled slice's late entries
 * included), so it is reusable.  NULL / 0-byte workspace: NF4DQ_OK (no split-K,
 * nothing to report).  Synchronous; call it after the calls it vouches for. */
int nf4_gemm_check_workspace(void* workspace, size_t workspace_bytes, void* hip_stream);

/* Human-readable text for a return code (static storage). */
const char* nf4_strerror(int code);

/* Library version string, e.g. "nf4dq 0.1.0 gfx950". */
const char* nf4_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NF4_DEQUANT_H_ */
