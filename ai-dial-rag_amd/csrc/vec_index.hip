// Host side of the vector index: handle lifetime, workspaces, kernel dispatch.
// C ABI declared in include/miretr.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "common.h"
#include "vec_blocks_host.h"
#include "vec_counted_copy.h"
#include "vec_kernels.h"
#include "vec_kernels_f16.h"
#include "vec_kernels_q16.h"
#include "vec_kernels_h16.h"
#include "vec_kernels_sieve.h"
#include "vec_kernels_i8.h"
#include "vec_kernels_exact.h"
#include "vec_kernels_scoped.h"
#include "vec_kernels_shared.h"
#include "vec_kernels_pieces.h"
#include "vec_kernels_expand.h"
#include "vec_scoped_layout.h"
#include "vec_pieces_layout.h"
#include "vec_frozen_layout.h"
#include "vec_fanout_layout.h"

namespace mir {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int32_t use_device(int32_t device, int *num_cus) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no usable HIP device (hipGetDeviceCount: %s); libmiretr has no CPU fallback",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        (void)hipGetLastError();
        return MIR_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (have %d)", device, count);
        return MIR_ERR_INVALID;
    }
    MIR_HIP(hipSetDevice(device));
    if (num_cus) {
        hipDeviceProp_t prop;
        MIR_HIP(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            set_error("device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
            return MIR_ERR_NO_DEVICE;
        }
        *num_cus = prop.multiProcessorCount;
    }
    return MIR_OK;
}

// k-steps (16 columns each) the register-resident scan is instantiated for
static int pad_ksteps(int d) {
    const int ks = (d + 15) / 16;
    static const int kInst[] = {1, 2, 4, 8, 16, 24};
    for (int v : kInst)
        if (ks <= v) return v;
    if (ks <= 32) return 32;  // 384 < d <= 1024: the 64-query K-split scan over the bf16 hi/lo image (whole 16-k-step stages)
    if (ks <= 48) return 48;
    if (ks <= 64) return 64;
    return (ks + 7) / 8 * 8;  // generic kernel: multiple of the ring depth
}

struct Workspace {
    hipStream_t stream = nullptr;    // own stream for the host-buffer API
    hipEvent_t done = nullptr;       // recorded after the last enqueue that used the buffers
    hipStream_t last_stream = nullptr;
    bool pending = false;
    void *buf = nullptr;             // one slab, carved below
    size_t cap = 0;
    char *pin = nullptr;             // pinned host staging of the host-buffer API: queries in, results out
    size_t pin_cap = 0;
};

}  // namespace mir

using namespace mir;

struct mir_index {
    int device = 0;
    int num_cus = 0;
    int64_t n = 0;
    int d = 0;
    int dtype = MIR_DTYPE_F32;
    int64_t row_offset = 0;
    int ksteps = 0;
    uint32_t n_tiles = 0;
    float *d_orig = nullptr;     // float32 rows (re-scoring); null on a float16-native index
    _Float16 *d_f16 = nullptr;   // float16-native index: the rows as given (re-scoring)
    bool native16 = false;       // float16 storage scanned as 2-byte fragments (vec_kernels_f16.h)
    bool layout16 = false;       // float32, d padded to 128 / 256 / 384: the 16x16x32 image of vec_kernels_q16.h
    bool hi_only = false;        // layout16 shard of sieve size (>= 32K rows: plan()): the image holds the bf16 hi blocks alone
    bool wide16 = false;         // float32, 384 < d <= 1024, of sieve size: `d_hi16` = the bf16 hi parts in the float16-native image's layout,
    int ks16 = 0;                //   ks16 blocks of 1 KiB per tile (d padded to 512 / 1024); the sieve's BF filter scans it, nothing reads d_split
    uint4 *d_hi16 = nullptr;
    uint4 *d_split = nullptr;    // bf16 hi/lo fragments, or the float16 fragments of a native16 index
    float *d_docsq = nullptr;    // padded to n_tiles*32
    float *d_invnorm = nullptr;  // padded to n_tiles*32
    float *d_dnorm = nullptr;    // max((float)|row|, 1e-8), exact_metric_wave's summation order: cosine_sim of the batched exact pass
    float *d_tilemax = nullptr;  // [n_tiles] a tile's largest row norm: the sieve's per-tile margin (layout16)
    bool norms_spread = false;   // the largest row norm exceeds the smallest tile maximum by more than 1/16 (or is not finite): the sieve takes its margins per tile /
                                 // per row (unit-norm embeddings - the headline - keep round 3's one margin per query: the per-tile form cost that step ~3 %)
    float *d_maxnorm = nullptr;
    // the sieve's int8 first stage (vec_kernels_i8.h): built after the float image where the shard qualifies (build_i8)
    bool i8 = false;
    uint4 *d_i8 = nullptr;       // n_stages x 2 tiles x ks64 * 2 blocks of 1 KiB
    float *d_i8stats = nullptr;  // kI8StatWords floats
    float4 *d_i8tp = nullptr;    // [n_stages * 2] tile parameters (scale, residual bound, 1 / (2 scale))
    float *d_i8rec = nullptr;    // [2][n_stages][72] the filter's per-stage records: squared norms + parameters, inverse norms + parameters
    int ks64 = 0;
    uint32_t n_stages = 0;       // 64-row stages = ceil(n_tiles / 2)
    unsigned long long *d_stats = nullptr;  // 8 counters of the sieve (mir_index_scan_stats)
    int64_t *d_chunk = nullptr;
    int32_t *d_doc = nullptr;
    int64_t hbm_bytes = 0;
    std::mutex mu;
    std::vector<Workspace *> pool;
    // benchmark instrumentation (mir_index_profile)
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    std::vector<hipEvent_t> prof_free;  // recycled events: hipEventCreate inside a timed loop costs milliseconds now and then
    int64_t prof_launches = 0;
    double prof_ms = 0.0;
};

// One document's rows resident in HBM (mir_rows_create): the unit that outlives requests, so that an
// index over ANY set of documents is composed device-to-device (mir_index_create_from_rows).
struct mir_rows {
    int device = 0;
    int64_t n = 0;
    int d = 0;
    int dtype = MIR_DTYPE_F32;
    void *d_emb = nullptr;       // n x d, as given (float32 or float16)
    int64_t *d_chunk = nullptr;  // n
    float *d_docsq = nullptr;    // n: float32 squared norms, bit for bit an index's d_docsq of these rows (mir_blocks_search)
    int64_t hbm_bytes = 0;
};

// The fan-out of one row block resident in HBM (mir_fanout_create; vec_fanout_layout.h): stored row r stands for the expanded
// rows at positions d_pos[d_ptr[r] .. d_ptr[r + 1]) with the chunk ids d_chunk[...] there.
struct mir_fanout {
    int device = 0;
    int64_t n = 0;               // stored rows
    int64_t R = 0;               // replicas = rows of the expanded block
    int64_t *d_ptr = nullptr;    // n + 1 (one entry, 0, for an empty block: a fan-out's rep_ptr is never null)
    int64_t *d_chunk = nullptr;  // R
    int64_t *d_pos = nullptr;    // R
    int64_t hbm_bytes = 0;
};

// A searcher over row blocks (mir_blocks_search): a row-less mir_index, held for its device, shape and workspace pool.
struct mir_blocks {
    mir_index *ix = nullptr;
};

namespace mir {

static void free_index(mir_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    for (Workspace *w : ix->pool) {
        if (w->pending) (void)hipEventSynchronize(w->done);
        if (w->buf) (void)hipFree(w->buf);
        if (w->pin) (void)hipHostFree(w->pin);
        if (w->done) (void)hipEventDestroy(w->done);
        if (w->stream) (void)hipStreamDestroy(w->stream);
        delete w;
    }
    for (auto &pr : ix->prof_events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (hipEvent_t ev : ix->prof_free) (void)hipEventDestroy(ev);
    (void)hipFree(ix->d_orig);
    (void)hipFree(ix->d_f16);
    (void)hipFree(ix->d_split);
    (void)hipFree(ix->d_docsq);
    (void)hipFree(ix->d_invnorm);
    (void)hipFree(ix->d_dnorm);
    (void)hipFree(ix->d_tilemax);
    (void)hipFree(ix->d_i8);
    (void)hipFree(ix->d_i8stats);
    (void)hipFree(ix->d_i8tp);
    (void)hipFree(ix->d_i8rec);
    (void)hipFree(ix->d_hi16);
    (void)hipFree(ix->d_maxnorm);
    (void)hipFree(ix->d_stats);
    (void)hipFree(ix->d_chunk);
    (void)hipFree(ix->d_doc);
    delete ix;
}

// The sieve's threshold sample: kSampleWgs workgroups x up to kSampleTilesPerWg tiles (32K rows)
constexpr int kSampleWgs = 256;
constexpr int kSampleTilesPerWg = 4;  // (8 / 16 / 32 tiles per workgroup measured within 0.5 % on 10M x 384, 1-4 % slower on 6.25M x 1024 float16)
// The sieve's filter launches (plan()): 256 queries per launch - two query tiles per wave - when a layout16 batch has more than
// 128 (the stream of a pass is the same, the matrix work doubles); shards of >= kSieveTwoLaunchTiles tiles per workgroup in two
// launches, the first over 1/kSieveFirstDiv of the tiles, but not fewer than kSieveFirstMinTiles (~157K rows) nor more than 1/4
constexpr int kSieveMaxQueriesPerLaunch = 256;
constexpr int kSieveTwoLaunchTiles = 64;
constexpr uint32_t kSieveFirstDiv = 16;
constexpr uint32_t kSieveFirstMinTiles = 4896;
constexpr int kI8FourWaveQueries = 65;  // the int8 filter runs four waves per workgroup from this many queries per launch (launch_sieve_i8)

// float32 index with 384 < d <= 1024: scanned 64 queries per pass by the K-split kernel of vec_kernels_f16.h
static bool wide64_split(const mir_index *ix) { return !ix->native16 && (ix->ksteps == 32 || ix->ksteps == 48 || ix->ksteps == 64); }
// >= 32K rows: there is a sample to take the sieve's first threshold from
static bool sieve_sized(const mir_index *ix) { return ix->n_tiles >= 4u * kSampleWgs; }

// f(std::integral_constant<int, KIND>) for the scan kind `metric` ranks by (euclidean_dist ranks as squared L2)
template <typename F>
static int32_t with_kind(int metric, F f) {
    if (metric == MIR_METRIC_INNER_PRODUCT) return f(std::integral_constant<int, SCAN_IP>{});
    if (metric == MIR_METRIC_COSINE_SIM) return f(std::integral_constant<int, SCAN_COS>{});
    return f(std::integral_constant<int, SCAN_L2>{});
}

// Build the derived device state from ix->d_orig (already filled) on `stream`.
// doc_sq / inv_norm / max norm: rows staged through LDS when at least 32 of them fit (d <= 511), else one thread
// per row (measured at d = 1024: 15 rows per workgroup, 37 ms per 6.25M rows against ~18 ms direct)
template <typename T>
static void launch_row_norms(const T *src, int64_t n, int d, mir_index *ix, hipStream_t stream) {
    unsigned int *mx = reinterpret_cast<unsigned int *>(ix->d_maxnorm);
    const int rows_per_wg = std::min<int64_t>(128, kNormsLdsBytes / ((int64_t)norms_row_stride(d) * 4));
    if (rows_per_wg >= 32) {
        const size_t lds = (size_t)rows_per_wg * norms_row_stride(d) * 4;
        row_norms_lds_kernel<T><<<dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg)), dim3(256), lds, stream>>>(
            src, n, d, rows_per_wg, ix->d_docsq, ix->d_invnorm, mx);
    } else {
        row_norms_kernel<T><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(src, n, d, ix->d_docsq, ix->d_invnorm, mx);
    }
}

static int32_t build_derived(mir_index *ix, hipStream_t stream) {
    const int64_t n = ix->n;
    const int d = ix->d;
    ix->ksteps = ix->native16 ? (d + 511) / 512 * 32 : pad_ksteps(d);  // native16: whole 32-k-step stages
    ix->layout16 = !ix->native16 && (ix->ksteps == 8 || ix->ksteps == 16 || ix->ksteps == 24);  // d padded to 128 / 256 / 384
    ix->n_tiles = (uint32_t)((n + kTileRows - 1) / kTileRows);
    // A layout16 shard of >= 32K rows is scanned by the sieve alone (plan(): k <= 64 -> sieve, beyond -> the exact pass), and the
    // sieve reads only the hi blocks: no lo blocks are stored for it - 7.68 GB at 10M x 384 - and a tile's
    // hi blocks follow the previous tile's directly, so the filter's stream is contiguous.  plan() routes on these same flags.
    ix->hi_only = ix->layout16 && sieve_sized(ix);
    // wide float32 shards of >= 32K rows: the sieve's bf16 filter over a hi-only image of its own (round 4); the hi/lo split image
    // of the K-split list scan is then never read (k <= 64 -> sieve, beyond -> the exact pass) and is not built
    ix->wide16 = wide64_split(ix) && sieve_sized(ix);
    ix->ks16 = ix->wide16 ? (d + 511) / 512 * 32 : 0;
    const size_t split_bytes = ix->wide16 ? 16 : (size_t)ix->n_tiles * ix->ksteps * ((ix->native16 || ix->hi_only) ? 1024 : 2048);
    const size_t aux_bytes = (size_t)(ix->n_tiles + 1) * kTileRows * sizeof(float);  // (one tile more: the int8 filter reads 64-row stages)
    MIR_HIP(hipMalloc(&ix->d_split, std::max<size_t>(split_bytes, 16)));
    MIR_HIP(hipMalloc(&ix->d_docsq, std::max<size_t>(aux_bytes, 16)));
    MIR_HIP(hipMalloc(&ix->d_invnorm, std::max<size_t>(aux_bytes, 16)));
    MIR_HIP(hipMalloc(&ix->d_maxnorm, 32));  // norm statistics: [0] largest norm, [1] non-finite flag, [2] largest bf16 residual, [3] largest residual / norm, [4] smallest tile maximum (bits), [5..7] -
    MIR_HIP(hipMalloc(&ix->d_dnorm, std::max<size_t>((size_t)n * 4, 16)));
    ix->hbm_bytes += split_bytes + 2 * aux_bytes + 32 + (size_t)n * 4;
    MIR_HIP(hipMemsetAsync(ix->d_docsq, 0, std::max<size_t>(aux_bytes, 16), stream));
    MIR_HIP(hipMemsetAsync(ix->d_invnorm, 0, std::max<size_t>(aux_bytes, 16), stream));
    MIR_HIP(hipMemsetAsync(ix->d_maxnorm, 0, 32, stream));
    MIR_HIP(hipMemsetAsync(reinterpret_cast<char *>(ix->d_maxnorm) + 16, 0xff, 4, stream));  // word 4: a minimum over unsigned float bits
    MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_stats), 64));
    MIR_HIP(hipMemsetAsync(ix->d_stats, 0, 64, stream));
    if (n > 0) {
        const int64_t total_lanes = (int64_t)ix->n_tiles * ix->ksteps * 64;
        const int64_t blocks = (total_lanes + 255) / 256;
        MIR_REQUIRE(blocks < (int64_t)0x7fffffff, "index too large for one pack launch");
        if (ix->native16) {
            pack_f16_16_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(ix->d_f16, n, d, ix->ksteps / 2, total_lanes,
                                                                               ix->d_split);  // a tile: ksteps blocks of 1 KiB
            MIR_HIP(hipGetLastError());
            launch_row_norms(ix->d_f16, n, d, ix, stream);
        } else if (ix->layout16) {
            const int64_t lanes16 = total_lanes;  // tiles x (ks32 * 2) blocks x 64 lanes; one thread writes a hi and a lo block
            pack_split16_f32_kernel<<<dim3((unsigned)((lanes16 + 255) / 256)), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->ksteps / 2,
                                                                                                   lanes16, ix->d_split, ix->hi_only);
            MIR_HIP(hipGetLastError());
            launch_row_norms(ix->d_orig, n, d, ix, stream);
        } else if (ix->wide16) {
            const int64_t lanes = (int64_t)ix->n_tiles * ix->ks16 * 64;
            MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_hi16), (size_t)ix->n_tiles * ix->ks16 * 1024));
            ix->hbm_bytes += (size_t)ix->n_tiles * ix->ks16 * 1024;
            pack_hi16_f32_kernel<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->ks16 / 2, lanes, ix->d_hi16);
            MIR_HIP(hipGetLastError());
            launch_row_norms(ix->d_orig, n, d, ix, stream);
        } else {
            pack_split_f32_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->ksteps,
                                                                                  total_lanes, ix->d_split);
            MIR_HIP(hipGetLastError());
            launch_row_norms(ix->d_orig, n, d, ix, stream);
        }
        MIR_HIP(hipGetLastError());
        if (ix->native16) row_dnorm_kernel<_Float16><<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream>>>(ix->d_f16, n, d, ix->d_dnorm);
        else row_dnorm_kernel<float><<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->d_dnorm);
        MIR_HIP(hipGetLastError());
        if (ix->layout16) {  // the sieve's per-tile margin (vec_kernels_q16.h, hihi_coeff)
            MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_tilemax), (size_t)ix->n_tiles * 4));
            ix->hbm_bytes += (size_t)ix->n_tiles * 4;
            tile_maxnorm_kernel<<<dim3((ix->n_tiles + 255) / 256), dim3(256), 0, stream>>>(ix->d_dnorm, n, ix->n_tiles, ix->d_tilemax,
                                                                                            reinterpret_cast<unsigned int *>(ix->d_maxnorm) + 4);
            MIR_HIP(hipGetLastError());
        }
    }
    return MIR_OK;
}

// The int8 image of a shard the bf16 sieve serves, where its one-scale-per-index quantisation and one-margin-per-query bound
// apply: finite rows, norms not spread (vec_kernels_i8.h).  Runs after build_derived's statistics are known on the host.
static int32_t build_i8(mir_index *ix, hipStream_t stream) {
    const int64_t n = ix->n;
    const int d = ix->d;
    ix->ks64 = ix->ksteps / 4;  // ksteps counts 16 columns: 8 / 16 / 24 -> 2 / 4 / 6 k-steps of 64
    ix->n_stages = (ix->n_tiles + 1) / 2;
    const size_t image = (size_t)ix->n_stages * 2 * ix->ks64 * 2 * 1024;
    MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_i8), image));
    MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_i8stats), kI8StatWords * 4));
    MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_i8tp), (size_t)ix->n_stages * 2 * 16));
    ix->hbm_bytes += image + kI8StatWords * 4 + (size_t)ix->n_stages * 2 * 16;
    MIR_HIP(hipMemsetAsync(ix->d_i8stats, 0, kI8StatWords * 4, stream));
    i8_tile_scale_kernel<<<dim3(ix->n_stages * 2), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->d_i8tp);
    i8_scale_kernel<<<dim3(1), dim3(1), 0, stream>>>(ix->d_i8stats, ix->d_maxnorm);
    const int64_t lanes = (int64_t)ix->n_stages * 2 * ix->ks64 * 2 * 64;
    pack_i8_kernel<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->ks64, lanes, ix->d_i8tp, ix->d_i8);
    i8_residual_kernel<<<dim3((unsigned)((n + 15) / 16)), dim3(256), 0, stream>>>(ix->d_orig, n, d, ix->d_docsq, ix->d_i8tp, ix->d_i8stats);
    MIR_HIP(hipGetLastError());
    float st[kI8StatWords] = {};
    MIR_HIP(hipMemcpyAsync(st, ix->d_i8stats, sizeof(st), hipMemcpyDeviceToHost, stream));
    MIR_HIP(hipStreamSynchronize(stream));
    // the integer test takes the smallest squared norm for every row's: rows of ONE norm only (normalised embeddings)
    ix->i8 = st[7] > 0.f && st[1] - st[7] <= 1e-3f * st[1];
    if (ix->i8) {  // the norms' range, for cosine
        // (doc_sq is a float32 sum of d squares: 1e-4 covers its rounding many times over and costs the bound nothing)
        const float nr[3] = {sqrtf(st[7]) * (1.0f - 1e-4f), sqrtf(st[1]) * (1.0f + 1e-4f), 1.0f / (sqrtf(st[7]) * (1.0f - 1e-4f))};
        MIR_HIP(hipMemcpy(ix->d_i8stats + 4, nr, sizeof(nr), hipMemcpyHostToDevice));
    }
    if (!ix->i8) {
        (void)hipFree(ix->d_i8);
        (void)hipFree(ix->d_i8tp);
        ix->d_i8 = nullptr;
        ix->d_i8tp = nullptr;
        ix->hbm_bytes -= image + (size_t)ix->n_stages * 2 * 16;
    } else {
        const size_t rec = (size_t)ix->n_stages * 72 * 4;
        MIR_HIP(hipMalloc(reinterpret_cast<void **>(&ix->d_i8rec), 2 * rec));
        ix->hbm_bytes += 2 * rec;
        const int64_t n_col = (int64_t)(ix->n_tiles + 1) * kTileRows;  // (the columns are padded by a tile: build_derived)
        i8_stage_record_kernel<<<dim3(ix->n_stages), dim3(128), 0, stream>>>(ix->d_docsq, n_col, ix->d_i8tp, ix->d_i8rec);
        i8_stage_record_kernel<<<dim3(ix->n_stages), dim3(128), 0, stream>>>(ix->d_invnorm, n_col, ix->d_i8tp, ix->d_i8rec + (size_t)ix->n_stages * 72);
        MIR_HIP(hipGetLastError());
        MIR_HIP(hipStreamSynchronize(stream));
    }
    return MIR_OK;
}

static int32_t check_create_args(int64_t n, int32_t d, int32_t dtype, mir_index **out) {
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    MIR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n=%lld out of range [0, 2^31)", (long long)n);
    MIR_REQUIRE(d >= 1 && d <= 128 * 4096, "d=%d out of range", d);
    if (dtype != MIR_DTYPE_F32 && dtype != MIR_DTYPE_F16) {
        set_error("dtype %d not supported (float32 = 0, float16 = 1)", dtype);
        return MIR_ERR_UNSUPPORTED;
    }
    return MIR_OK;
}

struct SearchBuffers {
    double *q;       // [b][d]      (host API only)
    uint4 *qsplit;   // [ngroups][ksteps][2][64]
    double *q_sq;    // [b]
    double *q_err;   // [b] |q - bf16(q)|: what the hi fragments lose on the query's side (layout16; the sieve's margin)
    double *q_norm;  // [b]
    float *q_amax;   // [b] the int8 filter: a query's largest |q_i| (-1: not finite); its scales go to `qscale`
    float *qscale;   // [b] 1 / (query scale) of the float16-native scan
    uint64_t *part;  // [ngroups][nwg][qpw][klist]
    uint64_t *gthr;  // [ngroups][max(128, qpw)] the sieve's per-query thresholds; the control words below
                     // follow it in ONE allocation, which the prep kernel zeroes (ctl_words)
    int32_t *nflag;  // [2] number of queries handed to the exact pass
    uint32_t *arrive;  // [b] arrival counters of the exact pass
    int ctl_words;   // 64-bit words from gthr to the end of arrive
    int32_t *flagged;  // [b]
    double *bound_dist;  // [b] exact pass, k > 64: last result of the previous round
    uint32_t *bound_row; // [b]
    uint64_t *part_exact;  // [b][exact grid][64][2]
    double *qt;            // [ceil(b / 32)][d padded to 256][32]: the flagged queries, transposed, for the batched exact pass
    uint64_t *part_sample;  // the sieve's threshold sample: [kSampleWgs][qpw] x (2 floats, then their 2 rows), reused by every launch group (stream-ordered)
    // the sieve (vec_kernels_sieve.h): candidate regions of its two launches, the queries' verified lists
    uint64_t *sv_cand;      // [2][nwg][kSieveRegion]
    float *sv_candv;        // [2][nwg][kSieveRegion]
    uint32_t *sv_ccount;    // [2][nwg]
    SieveLists sv;          // rv / row [b][kSieveQueryCap]; count / over [b] live in the zeroed control block
    SearchOut out;          // host API staging of outputs
};

// How a search runs (plan()): `ngroups` launches of the filter scan, `qpw` queries each, on `nwg` workgroups
// with candidate lists of `klist`; exact_only = no filter scan at all (k beyond the lists): every query takes
// the exact pass.
struct SearchPlan {
    int ngroups = 0, nwg = 1, klist = 2, qpw = 32;
    int exact_grid = 1;       // workgroups of exact_topk_kernel
    bool exact_only = false;
    bool sieve = false;       // shard of sieve size: hi-only filter + exhaustive verification (vec_kernels_sieve.h); nwg = workgroups per launch
    uint32_t tiles_first = 0; // the sieve: tiles of the first of its two filter launches (0 = one launch)
    uint32_t sample_tpw = 0;  // the sieve's threshold sample: tiles per sample workgroup
};

// Lays a search's buffers out from `base` (null: sizes the slab only) and returns the bytes the slab needs
static size_t carve(SearchBuffers &sb, char *base, const mir_index *ix, int b, int k, const SearchPlan &pl, bool host_api) {
    const int ngroups = pl.ngroups, nwg = pl.nwg, klist = pl.klist, qpw = pl.qpw;
    const int d = ix->d, ksteps = std::max(ix->ksteps, ix->ks16);  // (a wide16 index's ks16 where that is larger)
    const bool i8 = ix->i8 && pl.sieve;  // the int8 first stage may serve this call (enqueue_search)
    Carver c{base};
    sb.q = host_api ? c.take<double>((size_t)b * d) : nullptr;
    sb.qsplit = c.take<uint4>((size_t)ngroups * (qpw / 32) * ksteps * 128);
    sb.q_sq = c.take<double>(b);
    sb.q_err = c.take<double>(b);
    sb.q_norm = c.take<double>(b);
    sb.q_amax = c.take<float>(i8 ? b : 0);
    sb.qscale = c.take<float>((size_t)ngroups * std::max(128, qpw));
    sb.part = c.take<uint64_t>(pl.sieve ? 0 : (size_t)ngroups * nwg * qpw * klist);  // per-workgroup lists of the list scans (the sieve has its own regions: 33.5 MB per launch group saved)
    // one zeroed control block: gthr | nflag | arrive[b] | sieve over[b] | sieve count[b][32]  (u32 arrays padded to u64)
    const size_t gthr_words = (size_t)ngroups * std::max(128, qpw), arrive_words = ((size_t)b + 1) / 2;
    const size_t count_words = pl.sieve ? (size_t)b * kSieveCountStride / 2 : 0;
    sb.ctl_words = (int)(gthr_words + 1 + 2 * arrive_words + count_words);
    sb.gthr = c.take<uint64_t>((size_t)sb.ctl_words);
    sb.nflag = base ? reinterpret_cast<int32_t *>(sb.gthr + gthr_words) : nullptr;
    sb.arrive = base ? reinterpret_cast<uint32_t *>(sb.gthr + gthr_words + 1) : nullptr;
    sb.sv.over = base ? reinterpret_cast<uint32_t *>(sb.gthr + gthr_words + 1 + arrive_words) : nullptr;
    sb.sv.count = base ? reinterpret_cast<uint32_t *>(sb.gthr + gthr_words + 1 + 2 * arrive_words) : nullptr;
    sb.flagged = c.take<int32_t>(b);
    sb.bound_dist = c.take<double>(b);
    sb.bound_row = c.take<uint32_t>(b);
    sb.part_exact = c.take<uint64_t>((size_t)b * pl.exact_grid * std::min(k, kExactRound) * 2);
    sb.qt = c.take<double>((size_t)((b + kXbQ - 1) / kXbQ) * xb_dpad(d) * kXbQ);
    sb.part_sample = c.take<uint64_t>(pl.sieve ? (size_t)kSampleWgs * std::max(128, qpw) * 2 : 0);  // the sieve's sample: two floats and their two rows per workgroup and query
    const size_t sv_q = pl.sieve ? (size_t)b * kSieveQueryCap : 0;
    const size_t region = i8 ? (size_t)kI8Region : (size_t)kSieveRegion;  // (the int8 filter: eight wave-private parts per workgroup)
    sb.sv_cand = c.take<uint64_t>(pl.sieve ? (size_t)2 * nwg * region : 0);
    sb.sv_candv = c.take<float>(pl.sieve ? (size_t)2 * nwg * region : 0);
    sb.sv_ccount = c.take<uint32_t>(pl.sieve ? (size_t)2 * nwg * (i8 ? 8 : 1) : 0);
    sb.sv.rv = c.take<float>(sv_q);
    sb.sv.row = c.take<uint32_t>(sv_q);
    sb.out = carve_out(c, b, k, host_api);
    return c.off + 256;
}

// Take a workspace that is safe to enqueue on `stream` (null = use its own).
static int32_t acquire_ws(mir_index *ix, hipStream_t stream, size_t need, Workspace **out) {
    Workspace *w = nullptr;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        for (size_t i = 0; i < ix->pool.size(); ++i) {
            Workspace *c = ix->pool[i];
            bool ok = !c->pending || (stream && c->last_stream == stream);
            if (!ok && hipEventQuery(c->done) == hipSuccess) {
                c->pending = false;
                ok = true;
            }
            if (ok) {
                w = c;
                ix->pool.erase(ix->pool.begin() + i);
                break;
            }
        }
    }
    if (!w) {
        w = new (std::nothrow) Workspace();
        MIR_REQUIRE(w != nullptr, "out of host memory");
        hipError_t e1 = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
        hipError_t e2 = hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
        if (e1 != hipSuccess || e2 != hipSuccess) {
            set_error("workspace stream/event creation failed");
            delete w;
            return MIR_ERR_HIP;
        }
    }
    if (w->cap < need) {
        if (w->pending) {
            (void)hipEventSynchronize(w->done);
            w->pending = false;
        }
        if (w->buf) (void)hipFree(w->buf);
        w->buf = nullptr;
        w->cap = 0;
        hipError_t e = hipMalloc(&w->buf, need);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) for search workspace failed: %s", need, hipGetErrorString(e));
            std::lock_guard<std::mutex> lk(ix->mu);
            ix->pool.push_back(w);
            return MIR_ERR_HIP;
        }
        w->cap = need;
    }
    *out = w;
    return MIR_OK;
}

static void release_ws(mir_index *ix, Workspace *w, hipStream_t used, bool pending) {
    w->last_stream = used;
    w->pending = pending;
    if (pending) (void)hipEventRecord(w->done, used);
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->pool.push_back(w);
}

// Size, acquire, carve, run, release.  `layout(base)` carves the call's slab from `base` and returns the bytes it needs (a null
// base: the size alone), so a call states its layout once.  `body(w, s)` enqueues on `s`: the caller's `stream` for the device
// forms, whose workspace goes back pending on it; the workspace's own for the host forms (host_api), which have synchronised it
// - after an error too - by the time the workspace goes back.
template <typename Layout, typename Body>
static int32_t with_workspace(mir_index *ix, hipStream_t stream, bool host_api, Layout layout, Body body) {
    Workspace *w = nullptr;
    int32_t rc = acquire_ws(ix, host_api ? nullptr : stream, layout(nullptr), &w);
    if (rc != MIR_OK) return rc;
    layout(static_cast<char *>(w->buf));
    hipStream_t s = host_api ? w->stream : stream;
    rc = body(w, s);
    release_ws(ix, w, s, !host_api);
    return rc;
}

// A HIP call that must succeed: sets the message and returns `on_fail` (the caller's clean-up, an expression) when it does not
#define MIR_TRY(call, on_fail)                                                                     \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            set_error("%s failed: %s", #call, hipGetErrorString(e_));                              \
            return on_fail;                                                                        \
        }                                                                                          \
    } while (0)

// One array of a host form's input: where it lies in the workspace's input span, and the caller's
struct HostPiece {
    const void *dev;
    const void *host;
    size_t bytes;
};

// The host forms' round trip on the workspace's stream `s`: the `pieces` go to their places in the device span [in0, in0 + in_bytes),
// `enqueue(out)` runs on the staging block `st` - null for each array the caller did not ask for - and the results land in `user`.
// One pinned staging buffer per workspace: the inputs go in through it and ALL result arrays come
// back in ONE copy of the contiguous [doc .. flags] span.  With pageable user buffers every
// hipMemcpyAsync is a synchronous staged copy of its own (~10-15 us each, six of them on the way
// out): on a 1k-row index they were most of a 195 us call.
template <typename Enqueue>
static int32_t host_round_trip(Workspace *w, hipStream_t s, const HostPiece *pieces, int npieces, void *in0, size_t in_bytes,
                               const SearchOut &st, const SearchOut &user, int b, int k, Enqueue enqueue) {
    auto bail = [&](int32_t code) {  // nothing of this call is in flight when the workspace goes back
        (void)hipStreamSynchronize(s);
        return code;
    };
    const size_t in_pad = (in_bytes + 255) & ~(size_t)255;
    const char *span0 = reinterpret_cast<const char *>(st.doc);
    const size_t span = (size_t)(reinterpret_cast<const char *>(st.flags) + (size_t)b * 4 - span0);
    if (w->pin_cap < in_pad + span) {
        if (w->pin) (void)hipHostFree(w->pin);
        w->pin = nullptr;
        w->pin_cap = 0;
        MIR_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->pin), in_pad + span, hipHostMallocDefault), bail(MIR_ERR_HIP));
        w->pin_cap = in_pad + span;
    }
    for (int i = 0; i < npieces; ++i)
        std::memcpy(w->pin + (static_cast<const char *>(pieces[i].dev) - static_cast<const char *>(in0)), pieces[i].host, pieces[i].bytes);
    MIR_TRY(hipMemcpyAsync(in0, w->pin, in_bytes, hipMemcpyHostToDevice, s), bail(MIR_ERR_HIP));
    const SearchOut out{user.doc ? st.doc : nullptr, user.chunk ? st.chunk : nullptr, user.row ? st.row : nullptr,
                        user.dist ? st.dist : nullptr, st.count, st.flags};
    const int32_t rc = enqueue(out);
    if (rc != MIR_OK) return bail(rc);
    char *res = w->pin + in_pad;
    MIR_TRY(hipMemcpyAsync(res, span0, span, hipMemcpyDeviceToHost, s), bail(MIR_ERR_HIP));
    MIR_TRY(hipStreamSynchronize(s), bail(MIR_ERR_HIP));
    auto at = [&](const void *dev_ptr) { return res + (reinterpret_cast<const char *>(dev_ptr) - span0); };
    // the kernels write a query's first count[q] entries alone: what the span holds past them is an earlier call's, and stays here
    const int32_t *count = reinterpret_cast<const int32_t *>(at(st.count));
    mir::counted_copy(user.doc, at(st.doc), count, b, k, 4);
    mir::counted_copy(user.chunk, at(st.chunk), count, b, k, 8);
    mir::counted_copy(user.row, at(st.row), count, b, k, 8);
    mir::counted_copy(user.dist, at(st.dist), count, b, k, 8);
    std::memcpy(user.count, at(st.count), (size_t)b * 4);
    if (user.flags) std::memcpy(user.flags, at(st.flags), (size_t)b * 4);
    return MIR_OK;
}

// a scan's per-row term: squared norms (L2), inverse norms (cosine), nothing (inner product)
template <int KIND>
static const float *scan_aux(const mir_index *ix) {
    return KIND == SCAN_L2 ? ix->d_docsq : KIND == SCAN_COS ? ix->d_invnorm : nullptr;
}

// Launch of a kernel with `lds` bytes of dynamic LDS
template <typename Kernel, typename... Args>
static int32_t launch_dyn(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    MIR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<grid, block, lds, stream>>>(args...);
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

template <int KIND>
static int32_t launch_scan(const mir_index *ix, const uint4 *qsplit_g, int nq, int klist, int nwg,
                           uint64_t *part_g, hipStream_t stream) {
    const float *aux = scan_aux<KIND>(ix);
    const size_t lds = ((size_t)klist * 256 + 32 * (size_t)klist) * 8;
    const uint32_t n_rows = (uint32_t)ix->n;
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(256), lds, stream, ix->d_split, aux, qsplit_g, n_rows, ix->n_tiles, nq, klist, part_g);
    };
    switch (ix->ksteps) {
        case 1: return go(scan_topk_kernel<1, KIND>);
        case 2: return go(scan_topk_kernel<2, KIND>);
        case 4: return go(scan_topk_kernel<4, KIND>);  // (8 / 16 / 24 k-steps = d padded to 128 / 256 / 384 are layout16 indexes: launch_scan_q16)
        default:
            return launch_dyn(scan_topk_generic_kernel<KIND>, dim3(nwg), dim3(256), lds, stream, ix->d_split, aux, qsplit_g, ix->ksteps,
                              n_rows, ix->n_tiles, nq, klist, part_g);
    }
}

// float32 layout16 scan: 128 queries per launch, 16 per wave (vec_kernels_q16.h)
template <int KIND>
static int32_t launch_scan_q16(const mir_index *ix, const uint4 *qsplit_g, const double *q_norm_g, int nq, int klist, int nwg,
                               uint64_t *part_g, hipStream_t stream) {
    const float *aux = scan_aux<KIND>(ix);
    const int ks32 = ix->ksteps / 2;
    const size_t lds = q16_lds_bytes(ks32, klist);
    const uint32_t n_rows = (uint32_t)ix->n;
    const bool five = q16_ring_stages(klist) == 5;  // ring stages: 5, else 4
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(512), lds, stream, ix->d_split, aux, qsplit_g, q_norm_g, ix->d_maxnorm, n_rows,
                          ix->n_tiles, nq, klist, part_g);
    };
    switch (ks32) {
        case 4: return five ? go(scan_topk_q16_kernel<4, KIND, 5>) : go(scan_topk_q16_kernel<4, KIND, 4>);
        case 8: return five ? go(scan_topk_q16_kernel<8, KIND, 5>) : go(scan_topk_q16_kernel<8, KIND, 4>);
        case 12: return five ? go(scan_topk_q16_kernel<12, KIND, 5>) : go(scan_topk_q16_kernel<12, KIND, 4>);
        default:
            set_error("internal: q16 scan has no instance for %d k-steps of 32", ks32);
            return MIR_ERR_UNSUPPORTED;
    }
}

// the sieve's filter launch over tiles [tile0, tile0 + n_tiles) (vec_kernels_sieve.h); sample = the threshold pre-pass
template <int KIND>
static int32_t launch_sieve(const mir_index *ix, int qpw, const uint4 *qsplit_g, const double *q_norm_g, const double *q_sq_g,
                            const double *q_err_g, int nq, int nwg,
                            uint32_t tile0, uint32_t n_tiles, int nan_guard, const uint64_t *gthr_g, uint64_t *cand, float *candv,
                            uint32_t *ccount, float *part_sample, bool sample, unsigned long long *stat, hipStream_t stream) {
    const float *aux = scan_aux<KIND>(ix);
    const int ks32 = ix->ksteps / 2;
    const size_t lds = sieve_lds_bytes(ks32);
    const uint32_t n_rows = (uint32_t)ix->n;
#define MIR_SIEVE_PICK(KS, P)                                                                                          \
    (qpw > 128 ? (sample ? sieve_q16_kernel<KS, KIND, true, 2, P> : sieve_q16_kernel<KS, KIND, false, 2, P>)           \
               : (sample ? sieve_q16_kernel<KS, KIND, true, 1, P> : sieve_q16_kernel<KS, KIND, false, 1, P>))
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(512), lds, stream, ix->d_split, aux, qsplit_g, q_norm_g, q_sq_g, q_err_g, ix->d_maxnorm,
                          n_rows, tile0, n_tiles, nq, nan_guard, gthr_g, cand, candv, ccount, part_sample, stat,
                          (uint32_t)(ks32 * 2 * 64), ix->d_tilemax);  // (a tile's hi blocks)
    };
    switch (ks32) {
        case 4: return go(ix->norms_spread ? MIR_SIEVE_PICK(4, true) : MIR_SIEVE_PICK(4, false));
        case 8: return go(ix->norms_spread ? MIR_SIEVE_PICK(8, true) : MIR_SIEVE_PICK(8, false));
        case 12: return go(ix->norms_spread ? MIR_SIEVE_PICK(12, true) : MIR_SIEVE_PICK(12, false));
        default:
            set_error("internal: the sieve has no instance for %d k-steps of 32", ks32);
            return MIR_ERR_UNSUPPORTED;
    }
#undef MIR_SIEVE_PICK
}

// the int8 filter's launch over 64-row stages [stage0, stage0 + n_stages) (vec_kernels_i8.h)
template <int KIND>
static int32_t launch_sieve_i8(const mir_index *ix, int qpw, const float *q_scale_g, const uint4 *qfrag_g, const double *q_norm_g,
                               const double *q_sq_g, const double *q_err_g, int nq, int nwg, uint32_t stage0, uint32_t n_stages,
                               int nan_guard, const uint64_t *gthr_g, uint64_t *cand, float *candv, uint32_t *ccount, float *part_sample,
                               bool sample, unsigned long long *stat, hipStream_t stream) {
    // from 65 queries per launch: four waves per workgroup (two or four query tiles each) and two workgroups per CU - 0.83 against
    // 0.92 ms per 128-query step at 10M x 384, 1.13-1.16 against 1.27-1.30 per 256; up to 64 queries half of four waves' query
    // tiles would be empty: eight waves with one tile each
    const bool four = nq >= kI8FourWaveQueries;
    const size_t lds = sieve_i8_lds_bytes(ix->ks64, four ? 4 : 8);
    const uint32_t n_rows = (uint32_t)ix->n;
    const int grid = (four && !sample) ? 2 * nwg : nwg;  // (the candidate parts are per wave: nwg x 8 of them either way)
#define MIR_I8_PICK(KS)                                                                                                \
    (four ? (qpw > 128 ? (sample ? sieve_i8_kernel<KS, KIND, true, 4, 4> : sieve_i8_kernel<KS, KIND, false, 4, 4>)     \
                       : (sample ? sieve_i8_kernel<KS, KIND, true, 2, 4> : sieve_i8_kernel<KS, KIND, false, 2, 4>))    \
          : (qpw > 128 ? (sample ? sieve_i8_kernel<KS, KIND, true, 2, 8> : sieve_i8_kernel<KS, KIND, false, 2, 8>)     \
                       : (sample ? sieve_i8_kernel<KS, KIND, true, 1, 8> : sieve_i8_kernel<KS, KIND, false, 1, 8>)))
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(grid), dim3(four ? 256 : 512), lds, stream, ix->d_i8,
                          ix->d_i8rec + (KIND == SCAN_COS ? (size_t)ix->n_stages * 72 : 0), qfrag_g, q_norm_g, q_sq_g, q_err_g, ix->d_i8stats,
                          q_scale_g, n_rows, stage0, n_stages, nq, nan_guard, gthr_g, cand, candv, ccount, part_sample, stat);
    };
    switch (ix->ks64) {
        case 2: return go(MIR_I8_PICK(2));
        case 4: return go(MIR_I8_PICK(4));
        case 6: return go(MIR_I8_PICK(6));
        default:
            set_error("internal: the int8 filter has no instance for %d k-steps of 64", ix->ks64);
            return MIR_ERR_UNSUPPORTED;
    }
#undef MIR_I8_PICK
}

// the float16-native sieve's filter launch (vec_kernels_sieve.h, sieve_h16_kernel)
// BF: the bf16 hi image of a wide float32 shard (ix->d_hi16, ix->ks16), the query fragments of prep_queries16_kernel, `q_err_g`
template <int KIND, bool BF = false>
static int32_t launch_sieve16(const mir_index *ix, const uint4 *qfrag_g, const float *qscale_g, const double *q_norm_g, const double *q_sq_g,
                              int nq, int nwg, uint32_t tile0, uint32_t n_tiles, int nan_guard, const uint64_t *gthr_g, uint64_t *cand,
                              float *candv, uint32_t *ccount, float *part_sample, bool sample, unsigned long long *stat, hipStream_t stream,
                              const double *q_err_g = nullptr) {
    const float *aux = scan_aux<KIND>(ix);
    const size_t lds = sieve16_lds_bytes();
    const uint32_t n_rows = (uint32_t)ix->n;
    const uint4 *image = BF ? ix->d_hi16 : ix->d_split;
    const int ks = BF ? ix->ks16 : ix->ksteps;
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(512), lds, stream, image, aux, qfrag_g, qscale_g, q_norm_g, q_sq_g, q_err_g, ix->d_maxnorm,
                          n_rows, tile0, n_tiles, nq, nan_guard, gthr_g, cand, candv, ccount, part_sample, stat);
    };
    if (ks == 64) return go(sample ? sieve_h16_kernel<32, KIND, true, BF> : sieve_h16_kernel<32, KIND, false, BF>);
    if (ks == 32) return go(sample ? sieve_h16_kernel<16, KIND, true, BF> : sieve_h16_kernel<16, KIND, false, BF>);
    set_error("internal: the float16 sieve has no instance for %d k-steps", ks);
    return MIR_ERR_UNSUPPORTED;
}

// float16-native scan: 128 queries per launch, 16 per wave, one float16 product per fragment (vec_kernels_h16.h)
template <int KIND>
static int32_t launch_scan_h16(const mir_index *ix, const uint4 *qfrag_g, const float *qscale_g, int nq, int klist, int nwg,
                               uint64_t *part_g, const uint64_t *gthr_g, hipStream_t stream) {
    const float *aux = scan_aux<KIND>(ix);
    const size_t lds = h16_lds_bytes(klist);
    const uint32_t n_rows = (uint32_t)ix->n;
    const int ns = h16_ring_stages(klist);
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(512 / H16_QT), lds, stream, ix->d_split, aux, qfrag_g, qscale_g, n_rows, 0, ix->n_tiles, nq,
                          klist, part_g, gthr_g);  // (zeroed thresholds: see the kernel)
    };
    // ksteps = 64: 512 < d <= 1024, 32 k-steps of 32 columns (128 VGPRs of query fragments per wave); 32: 256 < d <= 512
    if (ix->ksteps == 64)
        return ns == 4   ? go(scan_topk_h16_kernel<32, KIND, 4, H16_QT>)
               : ns == 3 ? go(scan_topk_h16_kernel<32, KIND, 3, H16_QT>)
                         : go(scan_topk_h16_kernel<32, KIND, 2, H16_QT>);
    if (ix->ksteps == 32)
        return ns == 4   ? go(scan_topk_h16_kernel<16, KIND, 4, H16_QT>)
               : ns == 3 ? go(scan_topk_h16_kernel<16, KIND, 3, H16_QT>)
                         : go(scan_topk_h16_kernel<16, KIND, 2, H16_QT>);
    set_error("internal: float16 scan has no instance for %d k-steps", ix->ksteps);
    return MIR_ERR_UNSUPPORTED;
}

// float32 rows with 384 < d <= 1024: the 64-query K-split scan over the bf16 hi/lo image
template <int KIND>
static int32_t launch_scan_f16(const mir_index *ix, const uint4 *qfrag_g, int nq, int klist, int nwg,
                               uint64_t *part_g, hipStream_t stream) {
    const float *aux = scan_aux<KIND>(ix);
    const size_t lds = f16_lds_bytes(klist);
    const uint32_t n_rows = (uint32_t)ix->n;
    auto go = [&](auto kern) {
        return launch_dyn(kern, dim3(nwg), dim3(512), lds, stream, ix->d_split, aux, qfrag_g, n_rows, ix->n_tiles, nq, klist, part_g);
    };
    switch (ix->ksteps) {
        case 32: return go(scan_topk_f16_kernel<32, KIND>);
        case 48: return go(scan_topk_f16_kernel<48, KIND>);
        case 64: return go(scan_topk_f16_kernel<64, KIND>);
        default:
            set_error("internal: wide split scan has no instance for %d k-steps", ix->ksteps);
            return MIR_ERR_UNSUPPORTED;
    }
}

static int32_t check_search_args(const mir_index *ix, const void *queries, int32_t b, int32_t k, int32_t metric,
                                 const int32_t *out_count) {
    MIR_REQUIRE(ix != nullptr, "index is NULL");
    MIR_REQUIRE(b >= 0, "b=%d is negative", b);
    MIR_REQUIRE(b == 0 || queries != nullptr, "queries is NULL");
    MIR_REQUIRE(k >= 1, "k=%d must be >= 1", k);
    MIR_REQUIRE(metric >= 0 && metric <= 3, "unknown metric %d", metric);
    MIR_REQUIRE(b == 0 || out_count != nullptr, "out_count is NULL");
    return MIR_OK;
}

// One search call as its routes see it: device-resident queries `dq`, results to `out`, everything enqueued on `stream`
struct SearchCall {
    mir_index *ix;
    const double *dq;
    int b, k, metric;
    const SearchBuffers &sb;
    const SearchPlan &pl;
    const SearchOut &out;
    hipStream_t stream;
    bool use_i8;  // the int8 first stage serves this call (enqueue_search)
};

// Event bracket around the dominant (full-shard) scan launches of a launch group, on an index that is being profiled
// (mir_index_profile).  begin() takes two events from ix->prof_free, or creates them, and records the first; end() records the
// second and appends the pair to ix->prof_events.  A bracket that goes away without end() - a launch inside it failed - puts
// its events back on ix->prof_free.
struct ProfileBracket {
    mir_index *ix;
    hipStream_t stream;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ProfileBracket(mir_index *ix_, hipStream_t stream_) : ix(ix_), stream(stream_) {}
    ProfileBracket(const ProfileBracket &) = delete;
    ProfileBracket &operator=(const ProfileBracket &) = delete;
    int32_t begin() {
        if (!ix->profiling) return MIR_OK;
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            if (ix->prof_free.size() >= 2) {
                ev0 = ix->prof_free.back(); ix->prof_free.pop_back();
                ev1 = ix->prof_free.back(); ix->prof_free.pop_back();
            }
        }
        if (!ev0) {
            MIR_HIP(hipEventCreate(&ev0));
            MIR_HIP(hipEventCreate(&ev1));
        }
        MIR_HIP(hipEventRecord(ev0, stream));
        return MIR_OK;
    }
    int32_t end() {
        if (!ev0) return MIR_OK;
        MIR_HIP(hipEventRecord(ev1, stream));
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->prof_events.emplace_back(ev0, ev1);
        ev0 = ev1 = nullptr;
        return MIR_OK;
    }
    ~ProfileBracket() {
        if (!ev0 && !ev1) return;
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ev0) ix->prof_free.push_back(ev0);
        if (ev1) ix->prof_free.push_back(ev1);
    }
};

// what the batched exact pass and the serial one (one or two flagged queries) are both told about a call: A = ExactBatchArgs / ExactArgs
template <typename A>
static void set_exact_args(A &a, const SearchCall &c, int round) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    a.docs = ix->d_orig; a.docs16 = ix->d_f16; a.doc_sq = ix->d_docsq; a.n_rows = (uint32_t)ix->n; a.d = ix->d; a.metric = c.metric;
    a.q_sq = sb.q_sq; a.nflag = sb.nflag; a.flagged = sb.flagged;
    a.k = c.k; a.round = round; a.list_stride = std::min(c.k, kExactRound); a.part = sb.part_exact; a.arrive = sb.arrive;
    a.bound_dist = sb.bound_dist; a.bound_row = sb.bound_row; a.chunk_ids = ix->d_chunk; a.doc_ids = ix->d_doc;
    a.row_offset = ix->row_offset; a.out_doc = c.out.doc; a.out_chunk = c.out.chunk; a.out_row = c.out.row; a.out_dist = c.out.dist;
    a.out_count = c.out.count; a.out_flags = c.out.flags;
}

// Round `round` of the exact pass over the flagged queries.  Device-gated: exits at once when no query was flagged.
static int32_t exact_pass(const SearchCall &c, int round) {
    const mir_index *ix = c.ix;
    ExactBatchArgs ea;
    set_exact_args(ea, c, round);
    ea.dnorm = ix->d_dnorm; ea.qt = c.sb.qt;
    ExactArgs es;  // the serial pass's view of the same buffers
    set_exact_args(es, c, round);
    es.q = c.dq; es.q_norm = c.sb.q_norm;
    const bool cosine = c.metric == MIR_METRIC_COSINE_SIM;
    const dim3 grid(c.pl.exact_grid), block(kXbThreads);
    if (ix->native16 && cosine) exact_pass_kernel<_Float16, true><<<grid, block, 0, c.stream>>>(ea, es);
    else if (ix->native16) exact_pass_kernel<_Float16, false><<<grid, block, 0, c.stream>>>(ea, es);
    else if (cosine) exact_pass_kernel<float, true><<<grid, block, 0, c.stream>>>(ea, es);
    else exact_pass_kernel<float, false><<<grid, block, 0, c.stream>>>(ea, es);
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

// k beyond the filter's candidate lists: no scan; every query is the reference's own computation.
// ceil(min(k, n) / 64) rounds, each one pass over the rows per query.
static int32_t enqueue_exact_only(const SearchCall &c) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    const int b = c.b, d = ix->d, gwords = sb.ctl_words;
    prep_queries_kernel<<<dim3(std::max(b, (gwords + 63) / 64)), dim3(64), 0, c.stream>>>(
        c.dq, b, d, ix->ksteps, 0, nullptr, sb.q_sq, sb.q_norm, reinterpret_cast<unsigned long long *>(sb.gthr), gwords);
    flag_all_kernel<<<dim3(b), dim3(256), 0, c.stream>>>(b, sb.nflag, sb.flagged, c.dq, d, c.metric, sb.q_norm, sb.qt);
    MIR_HIP(hipGetLastError());
    const int64_t found = std::min<int64_t>(c.k, ix->n);
    const int rounds = (int)std::max<int64_t>(1, (found + kExactRound - 1) / kExactRound);
    for (int r = 0; r < rounds; ++r) {
        int32_t rc = exact_pass(c, r);
        if (rc != MIR_OK) return rc;
    }
    return MIR_OK;
}

// Query preparation: the fragment image the call's first scan reads (one of five), the per-query norms, and the control block -
// the sieve's thresholds + the exact pass's control words - zeroed by the first blocks of the kernel
static int32_t prep_queries(const SearchCall &c) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    const hipStream_t stream = c.stream;
    const double *dq = c.dq;
    const int b = c.b, d = ix->d, ngroups = c.pl.ngroups, qpw = c.pl.qpw;
    unsigned long long *gz = reinterpret_cast<unsigned long long *>(sb.gthr);
    const int gwords = sb.ctl_words;
    if (c.use_i8) {
        const int ntiles16 = ngroups * (qpw / 16);
        prep_queries_i8_stats_kernel<<<dim3(std::max(b, (gwords + 63) / 64)), dim3(64), 0, stream>>>(dq, b, d, sb.q_sq, sb.q_norm, sb.q_amax, gz, gwords);
        prep_queries_i8_quant_kernel<<<dim3(ntiles16 * ix->ks64 + b), dim3(64), 0, stream>>>(dq, b, d, ix->ks64, ntiles16, sb.q_amax, sb.qsplit,
                                                                                            sb.q_err, sb.qscale);
    } else if (ix->layout16 && qpw >= kQ16Queries) {
        const int ks32 = ix->ksteps / 2, ntiles16 = ngroups * (qpw / 16);
        prep_queries16_kernel<<<dim3(std::max(ntiles16 * ks32 + b, (gwords + 63) / 64)), dim3(64), 0, stream>>>(
            dq, b, d, ks32, ntiles16, sb.qsplit, sb.q_sq, sb.q_norm, gz, gwords, sb.q_err);
    } else if (ix->wide16 && c.pl.sieve) {  // bf16 hi (and lo, unread) fragments of 16 queries x 32 columns, |q - bf16(q)|
        const int ks32 = ix->ks16 / 2, ntiles16 = ngroups * (kQ16Queries / 16);
        prep_queries16_kernel<<<dim3(std::max(ntiles16 * ks32 + b, (gwords + 63) / 64)), dim3(64), 0, stream>>>(
            dq, b, d, ks32, ntiles16, sb.qsplit, sb.q_sq, sb.q_norm, gz, gwords, sb.q_err);
    } else if (ix->native16) {
        const int ks32 = ix->ksteps / 2, ntiles16 = ngroups * (kQ16Queries / 16);
        query_stats_h16_kernel<<<dim3(std::max(b, (gwords + 63) / 64)), dim3(64), 0, stream>>>(dq, b, d, sb.q_sq, sb.q_norm, sb.qscale, gz, gwords);
        prep_queries_h16_kernel<<<dim3(ntiles16 * ks32), dim3(64), 0, stream>>>(dq, b, d, ks32, sb.qscale, sb.qsplit);
    } else {
        const int ntiles32 = ngroups * (qpw / 32);  // 32-query fragment tiles, padded to whole launches
        // (blocks past the fragment and per-query blocks only zero their 64 words and return)
        const int prep_blocks = std::max(ntiles32 * ix->ksteps + b, (gwords + 63) / 64);
        prep_queries_kernel<<<dim3(prep_blocks), dim3(64), 0, stream>>>(dq, b, d, ix->ksteps, ntiles32, sb.qsplit, sb.q_sq, sb.q_norm, gz, gwords);
    }
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

// One launch group of the sieve, queries [q0, q0 + nq) of the batch
struct SieveGroup {
    int g, q0, nq;
    int guard;       // euclidean_dist: NaN guard of the filter and the select
    uint64_t *gthr;  // the group's thresholds
};

// One filter launch of group `sg` over tiles [t0, t0 + nt) on `wgs` workgroups, candidates to cand / cv / cc; smp = the threshold sample
static int32_t sieve_filter(const SearchCall &c, const SieveGroup &sg, uint32_t t0, uint32_t nt, int wgs, uint64_t *cand, float *cv,
                            uint32_t *cc, bool smp) {
    mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    const hipStream_t stream = c.stream;
    const int g = sg.g, q0 = sg.q0, nq = sg.nq, guard = sg.guard, qpw = c.pl.qpw;
    uint64_t *gt = sg.gthr;
    const double *qn = sb.q_norm + q0, *qsq = sb.q_sq + q0, *qerr = sb.q_err + q0;
    float *ps = reinterpret_cast<float *>(sb.part_sample);
    unsigned long long *st = smp ? nullptr : ix->d_stats + (t0 ? 1 : 0);
    if (c.use_i8) {  // tiles -> 64-row stages: [t0 / 2, (t0 + nt + 1) / 2) (t0 is even or 0 wherever two launches meet: plan())
        const uint32_t s0 = t0 / 2, s1 = std::min<uint32_t>((t0 + nt + 1) / 2, ix->n_stages);
        const uint4 *qf = sb.qsplit + (size_t)g * (qpw / 16) * ix->ks64 * 64;
        return with_kind(c.metric, [&](auto kind) {
            return launch_sieve_i8<kind()>(ix, qpw, sb.qscale + q0, qf, qn, qsq, qerr, nq, wgs, s0, s1 - s0, guard, gt, cand, cv, cc, ps, smp, st, stream);
        });
    }
    if (ix->native16) {
        const uint4 *qs16 = sb.qsplit + (size_t)g * (kQ16Queries / 16) * (ix->ksteps / 2) * 64;  // native16: hi fragments only
        const float *qsc = sb.qscale + (size_t)g * qpw;
        return with_kind(c.metric, [&](auto kind) {
            return launch_sieve16<kind()>(ix, qs16, qsc, qn, qsq, nq, wgs, t0, nt, guard, gt, cand, cv, cc, ps, smp, st, stream);
        });
    }
    if (ix->wide16) {  // (fragments of group g: 8 query tiles x ks16 / 2 k-steps x (hi, lo) blocks)
        const uint4 *qw = sb.qsplit + (size_t)g * (kQ16Queries / 16) * (ix->ks16 / 2) * 128;
        return with_kind(c.metric, [&](auto kind) {
            return launch_sieve16<kind(), true>(ix, qw, nullptr, qn, qsq, nq, wgs, t0, nt, guard, gt, cand, cv, cc, ps, smp, st, stream, qerr);
        });
    }
    const uint4 *qs = sb.qsplit + (size_t)g * (qpw / 32) * ix->ksteps * 128;
    return with_kind(c.metric, [&](auto kind) {
        return launch_sieve<kind()>(ix, qpw, qs, qn, qsq, qerr, nq, wgs, t0, nt, guard, gt, cand, cv, cc, ps, smp, st, stream);
    });
}

// what the select kernel is told about group `sg` (its `mode` is set per phase)
static SieveSelectArgs sieve_select_args(const SearchCall &c, const SieveGroup &sg) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    SieveSelectArgs sa;
    sa.l = sb.sv; sa.q0 = sg.q0; sa.nq = sg.nq; sa.k = c.k; sa.metric = c.metric; sa.d = ix->d; sa.nan_guard = sg.guard;
    sa.rel_err = ix->native16 ? (float)kH16RelErr : kHiHiRelErr;
    sa.extra_slop = ix->wide16 ? wide_accum_slop(ix->ks16 * 16) : 0.f;
    sa.docs = ix->d_orig; sa.docs16 = ix->d_f16; sa.doc_sq = ix->d_docsq;
    sa.dnorm = (ix->native16 || !ix->norms_spread) ? nullptr : ix->d_dnorm;
    sa.q = c.dq; sa.q_sq = sb.q_sq; sa.q_norm = sb.q_norm; sa.max_norm = ix->d_maxnorm;
    sa.q_err = ix->native16 ? nullptr : sb.q_err;
    sa.i8_qscale = nullptr;
    sa.i8_tparam = nullptr;
    if (c.use_i8) {  // the margin of the int8 filter's values: its statistics, its query residuals and scales (i8_margin)
        sa.max_norm = ix->d_i8stats;
        sa.i8_qscale = sb.qscale;
        sa.i8_tparam = ix->d_i8tp;
        sa.dnorm = nullptr;
    }
    sa.gthr = reinterpret_cast<unsigned long long *>(sg.gthr);
    sa.chunk_ids = ix->d_chunk; sa.doc_ids = ix->d_doc; sa.row_offset = ix->row_offset;
    sa.out_doc = c.out.doc; sa.out_chunk = c.out.chunk; sa.out_row = c.out.row; sa.out_dist = c.out.dist; sa.out_count = c.out.count;
    sa.out_flags = c.out.flags; sa.nflag = sb.nflag; sa.flagged = sb.flagged; sa.stats = ix->d_stats; sa.qt = sb.qt;
    return sa;
}

// Launch group `g` of the sieve: sample -> threshold, then per filter launch: filter (hi blocks only) -> scatter to the queries'
// lists -> select (reference formula for the rows that can be among the first k): exact by construction
static int32_t enqueue_sieve_group(const SearchCall &c, int g) {
    mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    const SearchPlan &pl = c.pl;
    const hipStream_t stream = c.stream;
    const int nwg = pl.nwg, qpw = pl.qpw, k = c.k;
    SieveGroup sg;
    sg.g = g; sg.q0 = qpw * g; sg.nq = std::min(qpw, c.b - qpw * g);
    sg.guard = c.metric == MIR_METRIC_EUCLIDEAN_DIST ? 1 : 0;
    sg.gthr = sb.gthr + (size_t)g * std::max(128, qpw);
    const int nq = sg.nq;
    unsigned long long *gt = reinterpret_cast<unsigned long long *>(sg.gthr);
    SieveScatterArgs ca;
    ca.q0 = sg.q0; ca.nq = nq; ca.l = sb.sv;
    SieveSelectArgs sa = sieve_select_args(c, sg);
    int32_t rc = sieve_filter(c, sg, 0, (uint32_t)kSampleWgs * pl.sample_tpw, kSampleWgs, nullptr, nullptr, nullptr, true);
    if (rc != MIR_OK) return rc;
    if (c.use_i8) {  // (the int8 filter's sample records its rows: T0 from their exact values)
        SieveSampleArgs ta;
        ta.part = reinterpret_cast<const float *>(sb.part_sample); ta.nwg = kSampleWgs; ta.qpw = qpw; ta.k = k; ta.nq = nq;
        ta.q0 = sg.q0; ta.d = ix->d; ta.metric = c.metric; ta.docs = ix->d_orig; ta.doc_sq = ix->d_docsq;
        ta.q = c.dq; ta.q_sq = sb.q_sq; ta.q_norm = sb.q_norm; ta.gthr = gt;
        sieve_sample_threshold_kernel<<<dim3(nq), dim3(256), 0, stream>>>(ta);
    } else {
        sample_threshold_kernel<<<dim3(nq), dim3(256), 0, stream>>>(reinterpret_cast<const float *>(sb.part_sample), kSampleWgs, qpw, k, nq, gt);
    }
    MIR_HIP(hipGetLastError());
    ProfileBracket prof(ix, stream);  // the bracket: both filter launches and what runs between them
    rc = prof.begin();
    if (rc != MIR_OK) return rc;
    for (int phase = pl.tiles_first ? 0 : 1; phase < 2; ++phase) {  // (one launch: the final phase alone)
        const size_t region = c.use_i8 ? (size_t)kI8Region : (size_t)kSieveRegion;
        uint64_t *cand = sb.sv_cand + (size_t)phase * nwg * region;
        float *cv = sb.sv_candv + (size_t)phase * nwg * region;
        uint32_t *cc = sb.sv_ccount + (size_t)phase * nwg * (c.use_i8 ? 8 : 1);
        rc = phase == 0 ? sieve_filter(c, sg, 0, pl.tiles_first, nwg, cand, cv, cc, false)
                        : sieve_filter(c, sg, pl.tiles_first, ix->n_tiles - pl.tiles_first, nwg, cand, cv, cc, false);
        if (rc == MIR_OK && phase == 1) rc = prof.end();
        if (rc != MIR_OK) return rc;
        ca.cand = cand; ca.candv = cv; ca.ccount = cc;
        if (c.use_i8) sieve_scatter_i8_kernel<<<dim3(nwg * 8), dim3(256), 0, stream>>>(ca);
        else sieve_scatter_kernel<<<dim3(nwg * kSieveScatterSplit), dim3(256), 0, stream>>>(ca);
        sa.mode = phase;
        rc = launch_dyn(sieve_select_kernel, dim3(nq), dim3(kSieveSelectThreads), sieve_select_lds_bytes(), stream, sa);
        if (rc != MIR_OK) return rc;
    }
    return MIR_OK;
}

// Launch group `g` of the list scans: one launch over the whole shard (every shard with a sample to seed thresholds from is the sieve's)
static int32_t enqueue_list_group(const SearchCall &c, int g) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    const hipStream_t stream = c.stream;
    const int nwg = c.pl.nwg, klist = c.pl.klist, qpw = c.pl.qpw, metric = c.metric;
    const uint4 *qs = sb.qsplit + (size_t)g * (qpw / 32) * ix->ksteps * 128;
    uint64_t *pg = sb.part + (size_t)g * nwg * qpw * klist;
    const int nq = std::min(qpw, c.b - qpw * g);
    ProfileBracket prof(c.ix, stream);
    int32_t rc = prof.begin();
    if (rc != MIR_OK) return rc;
    if (qpw == 32) {
        rc = with_kind(metric, [&](auto kind) { return launch_scan<kind()>(ix, qs, nq, klist, nwg, pg, stream); });
    } else if (ix->native16) {
        const uint4 *qs16 = sb.qsplit + (size_t)g * (kQ16Queries / 16) * (ix->ksteps / 2) * 64;  // hi fragments only
        const float *qsc = sb.qscale + (size_t)g * qpw;
        rc = with_kind(metric, [&](auto kind) { return launch_scan_h16<kind()>(ix, qs16, qsc, nq, klist, nwg, pg, sb.gthr + (size_t)g * 128, stream); });
    } else if (ix->layout16) {
        const double *qn = sb.q_norm + (size_t)g * qpw;
        rc = with_kind(metric, [&](auto kind) { return launch_scan_q16<kind()>(ix, qs, qn, nq, klist, nwg, pg, stream); });
    } else {  // wide64_split(ix): plan() gives 64 queries per launch to no other index
        rc = with_kind(metric, [&](auto kind) { return launch_scan_f16<kind()>(ix, qs, nq, klist, nwg, pg, stream); });
    }
    if (rc != MIR_OK) return rc;
    return prof.end();
}

// The list scans' last step: the workgroups' lists merged and re-scored into the results
static int32_t enqueue_finalize(const SearchCall &c) {
    const mir_index *ix = c.ix;
    const SearchBuffers &sb = c.sb;
    FinalizeArgs fa;
    fa.part = sb.part; fa.nwg = c.pl.nwg; fa.qpw = c.pl.qpw; fa.klist = c.pl.klist; fa.k = c.k; fa.b = c.b; fa.d = ix->d; fa.metric = c.metric;
    fa.docs = ix->d_orig; fa.docs16 = ix->d_f16; fa.doc_sq = ix->d_docsq; fa.max_norm = ix->d_maxnorm;
    fa.scan_rel_err = ix->native16 ? kH16RelErr : scan_rel_err(ix->d);  // the bound of the scan whose values the lists hold
    fa.q = c.dq; fa.q_sq = sb.q_sq; fa.q_norm = sb.q_norm;
    fa.chunk_ids = ix->d_chunk; fa.doc_ids = ix->d_doc; fa.row_offset = ix->row_offset;
    fa.out_doc = c.out.doc; fa.out_chunk = c.out.chunk; fa.out_row = c.out.row; fa.out_dist = c.out.dist;
    fa.out_count = c.out.count; fa.out_flags = c.out.flags; fa.nflag = sb.nflag; fa.flagged = sb.flagged; fa.qt = sb.qt;
    finalize_kernel<<<dim3(c.b), dim3(256), 0, c.stream>>>(fa);
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

// Enqueue prep + scan(s) + finalize for device-resident queries/outputs.
static int32_t enqueue_search(mir_index *ix, const double *dq, int b, int k, int metric, const SearchBuffers &sb,
                              const SearchPlan &pl, const SearchOut &out, hipStream_t stream) {
    // the int8 first stage serves this call: the shard has the image, the metric ranks in the rows' own units
    // ... and k is small: the int8 margin is 4.3 x the bf16 filter's, its lists grow with k (10M x 384: 4.2k candidates per query at k = 10,
    // 7.5k at 20, 11k at 32 - where the first queries overflow their 16384-entry lists and take the exact pass; the bf16 filter
    // lists 3.8k at k = 64) - beyond kI8MaxK the same index's bf16 image serves the call
    const bool use_i8 = ix->i8 && pl.sieve && sb.q_amax != nullptr && k <= kI8MaxK;
    const SearchCall c{ix, dq, b, k, metric, sb, pl, out, stream, use_i8};
    if (pl.exact_only) return enqueue_exact_only(c);
    int32_t rc = prep_queries(c);
    for (int g = 0; g < pl.ngroups && rc == MIR_OK; ++g) rc = pl.sieve ? enqueue_sieve_group(c, g) : enqueue_list_group(c, g);
    if (rc != MIR_OK) return rc;
    // the sieve's select kernel wrote the results; the list scans' come from finalize
    if (!pl.sieve) {
        rc = enqueue_finalize(c);
        if (rc != MIR_OK) return rc;
    }
    // queries whose buffers overflowed (the sieve) or whose candidate set finalize could not prove complete: exact pass, gated
    // on the device (it exits at once when there are none)
    return exact_pass(c, 0);
}

// How an index is searched.  Nothing but the index, b and k decides it:
//
//   index                                                   rows     k                path
//   layout16 (float32, d padded to 128 / 256 / 384),        >= 32K   <= 64            sieve
//   native16 (float16, 256 < d <= 1024),                    >= 32K   > 64             exact pass alone
//   wide float32 (384 < d <= 1024)                          < 32K    fits the lists   q16 / h16 / K-split list scan, one launch
//   everything else                                         any                       register-ring scans / exact pass
//
// 32K rows = 4 * kSampleWgs tiles (sieve_sized): from there the sieve has a sample to take its first threshold from, and the
// index build stores only the image the sieve reads (hi_only, wide16) - which is why the same flags route here.
static int32_t plan(const mir_index *ix, int b, int k, SearchPlan *pl) {
    // the exact pass: one workgroup of 16 waves per CU, one per 64-row block on small shards; its per-workgroup lists are
    // b x grid x min(k, 64) x 16 bytes of workspace - fewer workgroups for huge batches
    {
        const int64_t per_wg = (int64_t)b * std::min(k, kExactRound) * 16;
        const int64_t by_mem = std::max<int64_t>(64, ((int64_t)256 << 20) / std::max<int64_t>(per_wg, 1));
        pl->exact_grid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ix->num_cus, by_mem), (ix->n + kXbRows - 1) / kXbRows));
    }
    pl->klist = std::min(k + (ix->native16 ? kH16ListMargin : kListMargin), kMaxList);
    auto exact_only = [&]() {
        pl->exact_only = true;
        pl->ngroups = 0;
        pl->qpw = 32;
        pl->nwg = 1;
        return MIR_OK;
    };
    if (ix->hi_only || ix->wide16 || (ix->native16 && sieve_sized(ix))) {
        // filter on the hi blocks alone, verify every candidate; beyond the sieve's lists (k > 64, which no list scan holds
        // either) the exact pass alone
        if (k > kSieveMaxK) return exact_only();
        pl->sieve = true;
        pl->qpw = (ix->layout16 && b > kQ16Queries) ? kSieveMaxQueriesPerLaunch : kQ16Queries;
        pl->ngroups = (b + pl->qpw - 1) / pl->qpw;
        pl->nwg = (int)std::min<int64_t>(std::min(ix->num_cus, 1024), (int64_t)ix->n_tiles);
        pl->klist = std::min(k, kMaxList);
        // two filter launches on shards of >= kSieveTwoLaunchTiles tiles per workgroup: the second takes the exact k-th best
        // of the first as its threshold
        const bool two = (int64_t)ix->n_tiles >= (int64_t)kSieveTwoLaunchTiles * pl->nwg;
        pl->tiles_first = two ? std::max<uint32_t>(ix->n_tiles / kSieveFirstDiv, std::min<uint32_t>(ix->n_tiles / 4, kSieveFirstMinTiles)) : 0;
        pl->tiles_first &= ~1u;  // (the int8 filter walks 64-row stages: the two launches meet at a stage boundary)
        pl->sample_tpw = std::max<uint32_t>(1, std::min<uint32_t>(kSampleTilesPerWg, ix->n_tiles / (4u * kSampleWgs)));
        return MIR_OK;
    }
    // The reference takes any `limit` (embeddings_index.py:58,81).  Beyond what the filter's per-lane candidate
    // lists hold (LDS), an index that could actually return that many rows is searched by the exact pass alone.
    const bool wide64 = wide64_split(ix);
    const bool lists_fit = k + (ix->native16 ? kH16ListMargin : kListMargin) <= kMaxList;
    if (!lists_fit && ix->n > (int64_t)kMaxList) return exact_only();  // (n <= 64: every row fits the lists)
    if (wide64 && f16_lds_bytes(pl->klist) <= 160 * 1024) {  // 64 queries per pass; its LDS holds lists up to k = 28 (a float32
        pl->qpw = kF16Queries;                                  // index with a larger k falls through to the 32-query kernels)
        pl->ngroups = (b + pl->qpw - 1) / pl->qpw;
        const int64_t want16 = (int64_t)ix->n_tiles;
        pl->nwg = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ix->num_cus, 1024), want16));
        return MIR_OK;
    }
    if ((ix->layout16 || ix->native16) && pl->klist > kQ16MaxList) return exact_only();  // k > 52 (48 on a float16-native index) on a 16-queries-per-wave index (any n)
    if (ix->layout16 || ix->native16) {  // the images only the 16-queries-per-wave kernels read: they take every k their buffers hold (k <= 52; 48 on a float16-native index)
        pl->qpw = kQ16Queries;
        pl->ngroups = (b + pl->qpw - 1) / pl->qpw;
        pl->nwg = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ix->num_cus, 1024), (int64_t)ix->n_tiles));
        return MIR_OK;
    }
    pl->qpw = 32;  // the register-ring kernels: d <= 64, d > 1024, or a float32 wide index with k > 28
    pl->ngroups = (b + pl->qpw - 1) / pl->qpw;
    // one workgroup per CU, or one per tile on shards smaller than that: a workgroup's fixed costs
    // (ring start-up, filling empty lists) grow with the tiles it walks, and on a 1k-5k-row index one
    // tile per workgroup takes a single search from 128 to 90 us
    const int64_t want = (int64_t)ix->n_tiles;
    // (finalize's tournament gives each of its 256 threads up to 4 workgroup lists)
    pl->nwg = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ix->num_cus, 1024), want));
    return MIR_OK;
}

}  // namespace mir

// ============================================================ C ABI

// ---- composition of an index from per-document row blocks (all in HBM) ----
struct ConcatItem {
    const void *src;    // first unit of this piece
    int64_t dst_unit;   // where it goes, in units of the destination type
    int32_t n_units;    // <= kConcatPiece
    int32_t doc_id;     // for the doc-id fill (pieces are in row units there)
};
constexpr int kConcatPiece = 1 << 18;

template <typename U>
__global__ __launch_bounds__(256) void concat_kernel(const ConcatItem *__restrict__ items, U *__restrict__ dst) {
    const ConcatItem it = items[blockIdx.x];
    const U *src = static_cast<const U *>(it.src);
    U *out = dst + it.dst_unit;
    for (int i = threadIdx.x; i < it.n_units; i += 256) out[i] = src[i];
}
__global__ __launch_bounds__(256) void fill_doc_kernel(const ConcatItem *__restrict__ items, int32_t *__restrict__ dst) {
    const ConcatItem it = items[blockIdx.x];
    int32_t *out = dst + it.dst_unit;
    for (int i = threadIdx.x; i < it.n_units; i += 256) out[i] = it.doc_id;
}

// Where the rows of a new index come from: one matrix (host or device), or row blocks in HBM.
struct RowSource {
    const void *emb = nullptr;
    bool on_device = false;
    const int64_t *chunk_ids = nullptr;
    const int32_t *doc_ids = nullptr;
    const mir_rows *const *parts = nullptr;
    const int32_t *part_doc_ids = nullptr;
    int32_t nparts = 0;
};

// pieces of at most kConcatPiece units covering every part; unit_per_row units per row
static std::vector<ConcatItem> concat_items(const RowSource &src, int64_t units_per_row, size_t unit_bytes, int which) {
    std::vector<ConcatItem> items;
    int64_t row0 = 0;
    for (int p = 0; p < src.nparts; ++p) {
        const mir_rows *r = src.parts[p];
        const char *base = which == 0 ? static_cast<const char *>(r->d_emb) : reinterpret_cast<const char *>(r->d_chunk);
        const int64_t total = r->n * units_per_row;
        for (int64_t u = 0; u < total; u += kConcatPiece)
            items.push_back({base ? base + (size_t)u * unit_bytes : nullptr, row0 * units_per_row + u,
                             (int32_t)std::min<int64_t>(kConcatPiece, total - u), src.part_doc_ids ? src.part_doc_ids[p] : p});
        row0 += r->n;
    }
    return items;
}

template <typename Launch>
static hipError_t run_items(const std::vector<ConcatItem> &items, hipStream_t stream, Launch launch) {
    if (items.empty()) return hipSuccess;
    ConcatItem *d_items = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_items), items.size() * sizeof(ConcatItem));
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ConcatItem), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        launch(d_items, (unsigned)items.size());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // `items` (pageable) and d_items die here
    (void)hipFree(d_items);
    return e;
}

// rows of `src` -> dst (n x d elements of `esize` bytes)
static hipError_t copy_rows(const RowSource &src, void *dst, int64_t n, int32_t d, size_t esize, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!src.parts)
        return hipMemcpyAsync(dst, src.emb, (size_t)n * d * esize, src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream);
    const std::vector<ConcatItem> items = concat_items(src, d, esize, 0);
    return run_items(items, stream, [&](const ConcatItem *di, unsigned ni) {
        if (esize == 4) concat_kernel<uint32_t><<<dim3(ni), dim3(256), 0, stream>>>(di, static_cast<uint32_t *>(dst));
        else concat_kernel<uint16_t><<<dim3(ni), dim3(256), 0, stream>>>(di, static_cast<uint16_t *>(dst));
    });
}

extern "C" {

int32_t mir_abi_version(void) { return MIR_ABI_VERSION; }
const char *mir_last_error(void) { return mir::g_err; }

int32_t mir_device_count(int32_t *out_count) {
    MIR_REQUIRE(out_count != nullptr, "out_count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *out_count = c;
    return MIR_OK;
}

static int32_t create_common(const RowSource &src, int64_t n, int32_t d, int32_t dtype,
                             int32_t device, int64_t row_offset, hipStream_t stream, mir_index **out) {
    int32_t rc = check_create_args(n, d, dtype, out);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(n == 0 || src.emb != nullptr || src.parts != nullptr, "embeddings pointer is NULL");
    const int64_t *chunk_ids = src.chunk_ids;
    const int32_t *doc_ids = src.doc_ids;
    int cus = 0;
    rc = use_device(device, &cus);
    if (rc != MIR_OK) return rc;
    mir_index *ix = new (std::nothrow) mir_index();
    MIR_REQUIRE(ix != nullptr, "out of host memory");
    ix->device = device; ix->num_cus = cus; ix->n = n; ix->d = d; ix->dtype = dtype; ix->row_offset = row_offset;
    const hipMemcpyKind kind = src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto fail = [&](int32_t code) {
        free_index(ix);
        return code;
    };
    const size_t orig_bytes = (size_t)n * d * sizeof(float);
    // float16 rows with 256 < d <= 1024: kept as they are and scanned as 2-byte fragments, columns
    // zero-padded to 512 or 1024 (vec_kernels_h16.h); everything else goes through the float32 / bf16-split
    // layout (at d <= 256 the padding to 512 columns would scan as many bytes as that does)
    ix->native16 = dtype == MIR_DTYPE_F16 && d > 256 && d <= 1024;
    if (ix->native16) {
        MIR_TRY(hipMalloc(reinterpret_cast<void **>(&ix->d_f16), std::max<size_t>(orig_bytes / 2, 16)), fail(MIR_ERR_HIP));
        ix->hbm_bytes += orig_bytes / 2;
        MIR_TRY(copy_rows(src, ix->d_f16, n, d, 2, stream), fail(MIR_ERR_HIP));
    } else {
    MIR_TRY(hipMalloc(&ix->d_orig, std::max<size_t>(orig_bytes, 16)), fail(MIR_ERR_HIP));
    ix->hbm_bytes += orig_bytes;
    }
    if (ix->native16) {
    } else if (n > 0 && dtype == MIR_DTYPE_F32) {
        MIR_TRY(copy_rows(src, ix->d_orig, n, d, 4, stream), fail(MIR_ERR_HIP));
    } else if (n > 0) {
        // float16 input: widened exactly to float32 on the device.  Every float16 is hi + lo in
        // bfloat16 exactly (11 significant bits <= 8 + 8), so the scan is EXACT on such an index.
        void *tmp = nullptr;
        MIR_TRY(hipMalloc(&tmp, orig_bytes / 2), fail(MIR_ERR_HIP));
        hipError_t e1 = copy_rows(src, tmp, n, d, 2, stream);
        if (e1 == hipSuccess) {
            const int64_t total = n * (int64_t)d;
            widen_f16_kernel<<<dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, stream>>>(
                static_cast<const _Float16 *>(tmp), total, ix->d_orig);
            e1 = hipGetLastError();
        }
        if (e1 == hipSuccess) e1 = hipStreamSynchronize(stream);
        (void)hipFree(tmp);
        MIR_TRY(e1, fail(MIR_ERR_HIP));
    }
    if (src.parts && n > 0) {  // chunk ids of the blocks, doc id = the block's
        MIR_TRY(hipMalloc(&ix->d_chunk, (size_t)n * 8), fail(MIR_ERR_HIP));
        MIR_TRY(hipMalloc(&ix->d_doc, (size_t)n * 4), fail(MIR_ERR_HIP));
        ix->hbm_bytes += (size_t)n * 12;
        const std::vector<ConcatItem> items = concat_items(src, 1, 8, 1);
        MIR_TRY(run_items(items, stream, [&](const ConcatItem *di, unsigned ni) {
            concat_kernel<uint64_t><<<dim3(ni), dim3(256), 0, stream>>>(di, reinterpret_cast<uint64_t *>(ix->d_chunk));
            fill_doc_kernel<<<dim3(ni), dim3(256), 0, stream>>>(di, ix->d_doc);
        }), fail(MIR_ERR_HIP));
    }
    if (chunk_ids && n > 0) {
        MIR_TRY(hipMalloc(&ix->d_chunk, (size_t)n * 8), fail(MIR_ERR_HIP));
        MIR_TRY(hipMemcpyAsync(ix->d_chunk, chunk_ids, (size_t)n * 8, kind, stream), fail(MIR_ERR_HIP));
        ix->hbm_bytes += (size_t)n * 8;
    }
    if (doc_ids && n > 0) {
        MIR_TRY(hipMalloc(&ix->d_doc, (size_t)n * 4), fail(MIR_ERR_HIP));
        MIR_TRY(hipMemcpyAsync(ix->d_doc, doc_ids, (size_t)n * 4, kind, stream), fail(MIR_ERR_HIP));
        ix->hbm_bytes += (size_t)n * 4;
    }
    rc = build_derived(ix, stream);
    if (rc != MIR_OK) return fail(rc);
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        set_error("index build failed: %s", hipGetErrorString(e));
        return fail(MIR_ERR_HIP);
    }
    if (ix->d_tilemax) {  // (the build is complete: two floats of its norm statistics decide the sieve's margin form)
        float st[8] = {};
        e = hipMemcpy(st, ix->d_maxnorm, 32, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("index build failed: %s", hipGetErrorString(e));
            return fail(MIR_ERR_HIP);
        }
        ix->norms_spread = !(st[0] <= 1.0625f * st[4]);  // (NaN / infinite norms: spread)
        // the int8 first stage (vec_kernels_i8.h) serves the squared-L2 / euclidean / inner-product searches of a shard of finite rows
        // of one norm; MIR_SIEVE_I8=0 keeps the bf16 filter for everything (read per build, the library's one switch: the tests build
        // the same index with and without the image; it decides whether the image is BUILT - a search routes on ix->i8)
        const bool i8_on = !(getenv("MIR_SIEVE_I8") != nullptr && atoi(getenv("MIR_SIEVE_I8")) == 0);
        unsigned int nonfinite = 0;
        memcpy(&nonfinite, &st[1], 4);
        if (ix->hi_only && !ix->norms_spread && nonfinite == 0u && st[0] > 0.f && i8_on) {
            rc = build_i8(ix, stream);
            if (rc != MIR_OK) return fail(rc);
        }
    }
    *out = ix;
    return MIR_OK;
}

int32_t mir_index_create(const void *emb_host, int64_t n, int32_t d, int32_t dtype, const int64_t *chunk_ids_host,
                         const int32_t *doc_ids_host, int32_t device, int64_t row_offset, mir_index **out) {
    RowSource src;
    src.emb = emb_host; src.chunk_ids = chunk_ids_host; src.doc_ids = doc_ids_host;
    return create_common(src, n, d, dtype, device, row_offset, nullptr, out);
}

int32_t mir_index_create_from_device(const void *emb_device, int64_t n, int32_t d, int32_t dtype,
                                     const int64_t *chunk_ids_device, const int32_t *doc_ids_device,
                                     int32_t device, int64_t row_offset, void *stream, mir_index **out) {
    RowSource src;
    src.emb = emb_device; src.on_device = true; src.chunk_ids = chunk_ids_device; src.doc_ids = doc_ids_device;
    return create_common(src, n, d, dtype, device, row_offset, static_cast<hipStream_t>(stream), out);
}

// ---- row blocks ----
int32_t mir_rows_create(const void *emb_host, int64_t n, int32_t d, int32_t dtype, const int64_t *chunk_ids_host,
                        int32_t device, mir_rows **out) {
    mir_index *dummy = nullptr;
    int32_t rc = check_create_args(n, d, dtype, &dummy);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    MIR_REQUIRE(n == 0 || emb_host != nullptr, "embeddings pointer is NULL");
    rc = use_device(device, nullptr);
    if (rc != MIR_OK) return rc;
    mir_rows *r = new (std::nothrow) mir_rows();
    MIR_REQUIRE(r != nullptr, "out of host memory");
    r->device = device; r->n = n; r->d = d; r->dtype = dtype;
    const size_t eb = (size_t)n * d * (dtype == MIR_DTYPE_F16 ? 2 : 4);
    hipError_t e = hipSuccess;
    if (n > 0) {
        e = hipMalloc(&r->d_emb, eb);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->d_chunk), (size_t)n * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->d_docsq), (size_t)n * 4);
        if (e == hipSuccess) e = hipMemcpy(r->d_emb, emb_host, eb, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            if (chunk_ids_host) {
                e = hipMemcpy(r->d_chunk, chunk_ids_host, (size_t)n * 8, hipMemcpyHostToDevice);
            } else {  // NULL = 0..n-1, as mir_index_create
                std::vector<int64_t> ar((size_t)n);
                for (int64_t i = 0; i < n; ++i) ar[(size_t)i] = i;
                e = hipMemcpy(r->d_chunk, ar.data(), (size_t)n * 8, hipMemcpyHostToDevice);
            }
        }
        if (e == hipSuccess) {  // (the null stream: behind the copies above, done before this returns)
            const dim3 grid((unsigned)((n + 255) / 256));
            if (dtype == MIR_DTYPE_F16) row_sq_kernel<_Float16><<<grid, dim3(256)>>>(static_cast<const _Float16 *>(r->d_emb), n, d, r->d_docsq);
            else row_sq_kernel<float><<<grid, dim3(256)>>>(static_cast<const float *>(r->d_emb), n, d, r->d_docsq);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        }
        r->hbm_bytes = (int64_t)eb + n * 12;
    }
    if (e != hipSuccess) {
        set_error("mir_rows_create: %s", hipGetErrorString(e));
        (void)hipFree(r->d_emb); (void)hipFree(r->d_chunk); (void)hipFree(r->d_docsq);
        delete r;
        return MIR_ERR_HIP;
    }
    *out = r;
    return MIR_OK;
}

int32_t mir_rows_info(const mir_rows *rows, int64_t *n, int32_t *d, int32_t *dtype, int32_t *device, int64_t *hbm_bytes) {
    MIR_REQUIRE(rows != nullptr, "handle is NULL");
    if (n) *n = rows->n;
    if (d) *d = rows->d;
    if (dtype) *dtype = rows->dtype;
    if (device) *device = rows->device;
    if (hbm_bytes) *hbm_bytes = rows->hbm_bytes;
    return MIR_OK;
}

int32_t mir_rows_desc(const mir_rows *rows, mir_block_desc *out) {
    MIR_REQUIRE(rows != nullptr, "handle is NULL");
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = mir_block_desc{rows->d_emb, rows->d_docsq, rows->d_chunk, rows->n};
    return MIR_OK;
}

int32_t mir_rows_destroy(mir_rows *rows) {
    if (!rows) return MIR_OK;
    (void)hipSetDevice(rows->device);
    (void)hipFree(rows->d_emb);
    (void)hipFree(rows->d_chunk);
    (void)hipFree(rows->d_docsq);
    delete rows;
    return MIR_OK;
}

int32_t mir_index_create_from_rows(const mir_rows *const *parts, const int32_t *part_doc_ids, int32_t nparts,
                                   int32_t device, int64_t row_offset, mir_index **out) {
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    MIR_REQUIRE(nparts >= 1 && parts != nullptr, "no row blocks");
    int64_t n = 0;
    for (int p = 0; p < nparts; ++p) {
        MIR_REQUIRE(parts[p] != nullptr, "row block %d is NULL", p);
        MIR_REQUIRE(parts[p]->device == device, "row block %d lives on device %d, the index on %d", p, parts[p]->device, device);
        MIR_REQUIRE(parts[p]->d == parts[0]->d && parts[p]->dtype == parts[0]->dtype,
                    "row block %d is %d-dimensional dtype %d, block 0 is %d-dimensional dtype %d", p, parts[p]->d,
                    parts[p]->dtype, parts[0]->d, parts[0]->dtype);
        n += parts[p]->n;
    }
    RowSource src;
    src.on_device = true; src.parts = parts; src.part_doc_ids = part_doc_ids; src.nparts = nparts;
    return create_common(src, n, parts[0]->d, parts[0]->dtype, device, row_offset, nullptr, out);
}

int32_t mir_index_destroy(mir_index *idx) {
    free_index(idx);
    return MIR_OK;
}

int32_t mir_index_info(const mir_index *idx, int64_t *n, int32_t *d, int32_t *dtype, int32_t *device,
                       int64_t *hbm_bytes) {
    MIR_REQUIRE(idx != nullptr, "index is NULL");
    if (n) *n = idx->n;
    if (d) *d = idx->d;
    if (dtype) *dtype = idx->dtype;
    if (device) *device = idx->device;
    if (hbm_bytes) *hbm_bytes = idx->hbm_bytes;
    return MIR_OK;
}

int32_t mir_index_profile(mir_index *idx, int32_t enable) {
    MIR_REQUIRE(idx != nullptr, "index is NULL");
    if (enable) {
        int32_t rc = use_device(idx->device, nullptr);
        if (rc != MIR_OK) return rc;
        std::vector<hipEvent_t> fresh;
        for (int i = 0; i < 512; ++i) {  // enough for 256 launches between reads, created outside any timed region
            hipEvent_t ev = nullptr;
            MIR_HIP(hipEventCreate(&ev));
            fresh.push_back(ev);
        }
        std::lock_guard<std::mutex> lk(idx->mu);
        if (idx->prof_free.size() < 512) idx->prof_free.insert(idx->prof_free.end(), fresh.begin(), fresh.end());
        else for (hipEvent_t ev : fresh) (void)hipEventDestroy(ev);
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->profiling = enable != 0;
    return MIR_OK;
}

int32_t mir_index_profile_read(mir_index *idx, int32_t reset, int64_t *launches, double *total_ms) {
    MIR_REQUIRE(idx != nullptr, "index is NULL");
    int32_t rc = use_device(idx->device, nullptr);
    if (rc != MIR_OK) return rc;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    {
        std::lock_guard<std::mutex> lk(idx->mu);
        ev.swap(idx->prof_events);
    }
    double ms = 0.0;
    for (auto &pr : ev) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(pr.second);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, pr.first, pr.second);
        {
            std::lock_guard<std::mutex> lk(idx->mu);
            idx->prof_free.push_back(pr.first);
            idx->prof_free.push_back(pr.second);
        }
        if (e != hipSuccess) {
            set_error("profile read failed: %s", hipGetErrorString(e));
            return MIR_ERR_HIP;
        }
        ms += t;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->prof_launches += (int64_t)ev.size();
    idx->prof_ms += ms;
    if (launches) *launches = idx->prof_launches;
    if (total_ms) *total_ms = idx->prof_ms;
    if (reset) {
        idx->prof_launches = 0;
        idx->prof_ms = 0.0;
    }
    return MIR_OK;
}

// Counters of the sieve (large float32 shards, vec_kernels_sieve.h) since the last reset; synchronises the device.
// out[0], out[1]: (row, query) candidates its first / second filter launch wrote; out[2]: queries it answered;
// out[3]: queries it handed to the exact pass (a full buffer); out[4], out[5]: verified candidates that entered the
// ranking after the first launch / at the end.  out[6], out[7]: reserved (0).
int32_t mir_index_scan_stats(mir_index *idx, int32_t reset, int64_t *out8) {
    MIR_REQUIRE(idx != nullptr && out8 != nullptr, "NULL argument");
    int32_t rc = use_device(idx->device, nullptr);
    if (rc != MIR_OK) return rc;
    MIR_HIP(hipDeviceSynchronize());
    MIR_HIP(hipMemcpy(out8, idx->d_stats, 64, hipMemcpyDeviceToHost));
    if (reset) MIR_HIP(hipMemset(idx->d_stats, 0, 64));
    out8[6] = idx->i8 ? 1 : 0;  // the shard has the int8 image: its searches for up to kI8MaxK results use the int8 first stage
    return MIR_OK;
}

int32_t mir_index_search_device(mir_index *idx, const double *queries_device, int32_t b, int32_t k,
                                int32_t metric, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row,
                                double *out_dist, int32_t *out_count, int32_t *out_flags, void *stream_) {
    int32_t rc = check_search_args(idx, queries_device, b, k, metric, out_count);
    if (rc != MIR_OK) return rc;
    if (b == 0) return MIR_OK;
    rc = use_device(idx->device, nullptr);
    if (rc != MIR_OK) return rc;
    SearchPlan pl;
    rc = plan(idx, b, k, &pl);
    if (rc != MIR_OK) return rc;
    SearchBuffers sb;
    const SearchOut out{out_doc, out_chunk, out_row, out_dist, out_count, out_flags};
    return with_workspace(
        idx, static_cast<hipStream_t>(stream_), false, [&](char *base) { return carve(sb, base, idx, b, k, pl, false); },
        [&](Workspace *, hipStream_t s) { return enqueue_search(idx, queries_device, b, k, metric, sb, pl, out, s); });
}

int32_t mir_index_search(mir_index *idx, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                         int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                         int32_t *out_count, int32_t *out_flags) {
    int32_t rc = check_search_args(idx, queries_host, b, k, metric, out_count);
    if (rc != MIR_OK) return rc;
    if (b == 0) return MIR_OK;
    rc = use_device(idx->device, nullptr);
    if (rc != MIR_OK) return rc;
    SearchPlan pl;
    rc = plan(idx, b, k, &pl);
    if (rc != MIR_OK) return rc;
    SearchBuffers sb;
    const SearchOut user{out_doc, out_chunk, out_row, out_dist, out_count, out_flags};
    return with_workspace(
        idx, nullptr, true, [&](char *base) { return carve(sb, base, idx, b, k, pl, true); },
        [&](Workspace *w, hipStream_t s) {
            const size_t q_bytes = (size_t)b * idx->d * sizeof(double);
            const HostPiece in[] = {{sb.q, queries_host, q_bytes}};
            return host_round_trip(w, s, in, 1, sb.q, q_bytes, sb.out, user, b, k, [&](const SearchOut &out) {
                return enqueue_search(idx, sb.q, b, k, metric, sb, pl, out, s);
            });
        });
}

}  // extern "C"

// ---------------------------------------------------------------- scoped search (vec_kernels_scoped.h, vec_kernels_shared.h)
// Eight entries, one host path: an entry checks its arguments and fills a ScopedCall, run_scoped does the rest.

namespace mir {

struct ScopedCall {
    mir_index *ix;
    const double *queries;
    int b, k, metric;
    const int32_t *scope_ptr;
    const int64_t *seg_begin, *seg_end;  // the segments: row ranges of the index, or
    const mir_block_desc *table;         //   row blocks, one descriptor each (may be null where no scope lists a block:
    bool blocks;                         //   `blocks` says which search this is)
    SearchOut out;                 // the caller's
    hipStream_t stream = nullptr;  // the device forms: the caller's stream
    bool host_api = false;         // the host forms: every array above is the host's, and walk_scopes has filled
    ScopeRows rows{0, 0};          //   the segments of all scopes and the longest scope (0 = unknown)
    int n_groups = -1;             // >= 0: the shared search, scope_ptr per group, with
    const int32_t *group_ptr = nullptr;
    SharedPlan plan{};
    int max_slabs = 0;
    bool expanded = false;         // the expanded block search: `out` takes the expansion of the stream kernel's lists through
    const mir_fanout_desc *fan_table = nullptr;  // the fan-outs, one descriptor per block of `table` (null: none has one)
};

static int32_t check_scoped_args(const mir_index *ix, const void *queries, int32_t b, int32_t k, int32_t metric,
                                 const int32_t *scope_ptr, const int32_t *out_count) {
    int32_t rc = check_search_args(ix, queries, b, k, metric, out_count);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(b == 0 || scope_ptr != nullptr, "scope_ptr is NULL");
    return MIR_OK;
}

// The block searches' host forms, everything their device forms trust: scope_ptr, and each listed block against the searcher
// while it becomes its entry of the descriptor `table` the kernels read.  `unit`: what owns a scope, "query" or "group".
static int32_t check_blocks(const mir_index *ix, const int32_t *scope_ptr, int n_scopes, const char *unit, const int32_t *group_ptr,
                            const mir_rows *const *blocks, std::vector<mir_block_desc> &table, ScopeRows *rows) {
    int32_t rc = check_ptr_array(scope_ptr, n_scopes, "scope_ptr", unit);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(scope_ptr[n_scopes] == 0 || blocks != nullptr, "the block table is NULL");
    table.resize((size_t)scope_ptr[n_scopes]);
    return walk_scopes(scope_ptr, n_scopes, unit, group_ptr, [&](int t, int ordinal, int i, uint64_t *len) -> int32_t {
        const mir_rows *r = blocks[t];
        MIR_REQUIRE(r != nullptr, "block %d of %s %d is NULL", ordinal, unit, i);
        MIR_REQUIRE(r->d == ix->d && r->dtype == ix->dtype && r->device == ix->device,
                    "block %d of %s %d is %d-dimensional dtype %d on device %d, the searcher %d-dimensional dtype %d on device %d",
                    ordinal, unit, i, r->d, r->dtype, r->device, ix->d, ix->dtype, ix->device);
        table[(size_t)t] = mir_block_desc{r->d_emb, r->d_docsq, r->d_chunk, r->n};
        *len = (uint64_t)r->n;
        return MIR_OK;
    }, rows);
}

// mir_blocks_search's checks for a caller in another translation unit (vec_blocks_host.h)
int32_t blocks_check_host(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, const int32_t *scope_ptr_host,
                          const mir_rows *const *blocks_host, const int32_t *out_count, std::vector<mir_block_desc> *table, int32_t *d,
                          int32_t *device) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    const int32_t rc = check_scoped_args(s_->ix, queries_host, b, k, metric, scope_ptr_host, out_count);
    if (rc != MIR_OK) return rc;
    *d = s_->ix->d;
    *device = s_->ix->device;
    table->clear();
    if (b == 0) return MIR_OK;
    ScopeRows rows{0, 0};
    return check_blocks(s_->ix, scope_ptr_host, b, "query", nullptr, blocks_host, *table, &rows);
}

int32_t blocks_dim(const mir_blocks *s_) { return s_->ix->d; }

// mir_blocks_search_expanded's part past check_blocks: the fan-outs against their blocks, while they become the descriptor
// table the expansion reads (all null = the block has none); the expanded scopes' rows
static int32_t check_fanouts(const int32_t *scope_ptr_host, int32_t b, const mir_rows *const *blocks_host, const mir_fanout *const *fanouts_host,
                             size_t listed, std::vector<mir_fanout_desc> *fan_table) {
    fan_table->assign(listed, mir_fanout_desc{nullptr, nullptr, nullptr, 0});
    for (int i = 0; i < b; ++i) {
        uint64_t rows = 0;
        for (int t = scope_ptr_host[i]; t < scope_ptr_host[i + 1]; ++t) {
            const mir_fanout *f = fanouts_host ? fanouts_host[t] : nullptr;
            const int ordinal = t - scope_ptr_host[i];
            if (f) {
                MIR_REQUIRE(f->n == blocks_host[t]->n && f->device == blocks_host[t]->device,
                            "the fan-out of block %d of query %d is of %lld stored rows on device %d, the block holds %lld on device %d", ordinal, i,
                            (long long)f->n, f->device, (long long)blocks_host[t]->n, blocks_host[t]->device);
                (*fan_table)[(size_t)t] = mir_fanout_desc{f->d_ptr, f->d_chunk, f->d_pos, f->n};
            }
            rows += (uint64_t)(f ? f->R : blocks_host[t]->n);
            MIR_REQUIRE(rows < (1ull << 32), "the expanded scope of query %d holds 2^32 rows or more", i);
        }
    }
    return MIR_OK;
}

// mir_blocks_search_expanded's checks for a caller in another translation unit (vec_blocks_host.h)
int32_t blocks_expanded_check_host(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, const int32_t *scope_ptr_host,
                                   const mir_rows *const *blocks_host, const mir_fanout *const *fanouts_host, const int32_t *out_count,
                                   std::vector<mir_block_desc> *table, std::vector<mir_fanout_desc> *fan_table, int32_t *d, int32_t *device) {
    const int32_t rc = blocks_check_host(s_, queries_host, b, k, metric, scope_ptr_host, blocks_host, out_count, table, d, device);
    fan_table->clear();
    if (rc != MIR_OK || b == 0) return rc;
    return check_fanouts(scope_ptr_host, b, blocks_host, fanouts_host, table->size(), fan_table);
}

// mir_ensemble_scope_create's walk of one slot (vec_blocks_host.h): check_blocks and check_fanouts for ONE document list
int32_t scope_slot_check_host(int32_t slot, const mir_blocks *s_, const mir_rows *const *blocks, const mir_fanout *const *fanouts, int32_t n_docs,
                              int32_t device, mir_block_desc *desc, mir_fanout_desc *fan, bool *paged) {
    MIR_REQUIRE(s_ != nullptr, "the searcher of slot %d is NULL", slot);
    const mir_index *ix = s_->ix;
    MIR_REQUIRE(ix->device == device, "the searcher of slot %d is on device %d, the scope on device %d", slot, ix->device, device);
    MIR_REQUIRE(n_docs == 0 || blocks != nullptr, "the block table of slot %d is NULL", slot);
    *paged = false;
    uint64_t rows = 0, expanded = 0;
    for (int32_t t = 0; t < n_docs; ++t) {
        const mir_rows *r = blocks[t];
        MIR_REQUIRE(r != nullptr, "block %d of slot %d is NULL", t, slot);
        MIR_REQUIRE(r->d == ix->d && r->dtype == ix->dtype && r->device == ix->device,
                    "block %d of slot %d is %d-dimensional dtype %d on device %d, the searcher %d-dimensional dtype %d on device %d", t, slot, r->d,
                    r->dtype, r->device, ix->d, ix->dtype, ix->device);
        desc[t] = mir_block_desc{r->d_emb, r->d_docsq, r->d_chunk, r->n};
        rows += (uint64_t)r->n;
        MIR_REQUIRE(rows < (1ull << 32), "the scope of slot %d holds 2^32 rows or more", slot);
        const mir_fanout *f = fanouts ? fanouts[t] : nullptr;
        fan[t] = mir_fanout_desc{nullptr, nullptr, nullptr, 0};
        if (f) {
            MIR_REQUIRE(f->n == r->n && f->device == r->device,
                        "the fan-out of block %d of slot %d is of %lld stored rows on device %d, the block holds %lld on device %d", t, slot,
                        (long long)f->n, f->device, (long long)r->n, r->device);
            fan[t] = mir_fanout_desc{f->d_ptr, f->d_chunk, f->d_pos, f->n};
            *paged = true;
        }
        expanded += (uint64_t)(f ? f->R : r->n);
        MIR_REQUIRE(expanded < (1ull << 32), "the expanded scope of slot %d holds 2^32 rows or more", slot);
    }
    return MIR_OK;
}

// per-query norms (ngroups = 0: no fragments) + `counters` arrival counters zeroed
static void launch_scoped_prep(const ScopedCall &c, const ScopedBuffers &sb, int counters, hipStream_t stream) {
    const int arrive_words = (counters + 1) / 2;
    prep_queries_kernel<<<dim3(std::max(c.b, (arrive_words + 63) / 64)), dim3(64), 0, stream>>>(c.queries, c.b, c.ix->d, c.ix->ksteps, 0, nullptr, sb.q_sq,
                                                                                                  sb.q_norm, sb.arrive, arrive_words);
}

// The kernels' view of a call whose arrays are on the device (a block searcher's index holds no rows: null, 0)
static ScopedArgs scoped_args(const ScopedCall &c, const ScopedBuffers &sb, const SearchOut &out) {
    const mir_index *ix = c.ix;
    ScopedArgs a;
    a.docs = ix->d_orig; a.docs16 = ix->d_f16; a.doc_sq = ix->d_docsq; a.n_rows = (uint32_t)ix->n; a.d = ix->d; a.metric = c.metric;
    a.q = c.queries; a.q_sq = sb.q_sq; a.q_norm = sb.q_norm; a.q0 = 0; a.scope_ptr = c.scope_ptr; a.seg_begin = c.seg_begin; a.seg_end = c.seg_end; a.blocks = c.table;
    a.k = c.k; a.round = 0; a.list_stride = std::min(c.k, kExactRound); a.part = sb.part; a.arrive = reinterpret_cast<uint32_t *>(sb.arrive);
    a.bound_dist = sb.bound_dist; a.bound_pos = sb.bound_pos; a.chunk_ids = ix->d_chunk; a.row_offset = ix->row_offset;
    a.out_doc = out.doc; a.out_chunk = out.chunk; a.out_row = out.row; a.out_dist = out.dist; a.out_count = out.count; a.out_flags = out.flags;
    return a;
}

template <typename T, bool BLOCKS>
static void launch_scoped(const ScopedArgs &a, bool qlds, dim3 grid, size_t lds, hipStream_t stream) {
    if (qlds) scoped_topk_kernel<T, true, BLOCKS><<<grid, dim3(kScopedThreads), lds, stream>>>(a);
    else scoped_topk_kernel<T, false, BLOCKS><<<grid, dim3(kScopedThreads), lds, stream>>>(a);
}

static int32_t enqueue_scoped(const ScopedCall &c, int P, const ScopedBuffers &sb, const SearchOut &out, hipStream_t stream) {
    const mir_index *ix = c.ix;
    const int d = ix->d, b = c.b, k = c.k;
    const bool f16 = c.table ? ix->dtype == MIR_DTYPE_F16 : ix->d_f16 != nullptr;  // (blocks keep float16 as given at any d)
    launch_scoped_prep(c, sb, b, stream);
    ScopedArgs a = scoped_args(c, sb, out);
    const bool qlds = d <= kScopedLdsDim;
    const size_t lds = qlds ? (size_t)d * sizeof(double) : 0;
    constexpr int kSlice = 32768;  // queries per launch (grid.y)
    for (int round = 0; round * kExactRound < k; ++round) {
        a.round = round;
        for (int q0 = 0; q0 < b; q0 += kSlice) {
            a.q0 = q0;
            const dim3 grid((unsigned)P, (unsigned)std::min(kSlice, b - q0));
            if (c.table && f16) launch_scoped<_Float16, true>(a, qlds, grid, lds, stream);
            else if (c.table) launch_scoped<float, true>(a, qlds, grid, lds, stream);
            else if (f16) launch_scoped<_Float16, false>(a, qlds, grid, lds, stream);
            else launch_scoped<float, false>(a, qlds, grid, lds, stream);
        }
    }
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

template <typename T>
static int32_t launch_shared(const SharedArgs &a, const SharedPlan &pl, dim3 grid, hipStream_t stream) {
    const dim3 block(kScopedThreads);
    if (pl.qs == 64) return launch_dyn(shared_topk_kernel<T, 4, true>, grid, block, pl.lds, stream, a);
    if (pl.qs == 32) return launch_dyn(shared_topk_kernel<T, 2, true>, grid, block, pl.lds, stream, a);
    if (pl.qlds) return launch_dyn(shared_topk_kernel<T, 1, true>, grid, block, pl.lds, stream, a);
    return launch_dyn(shared_topk_kernel<T, 1, false>, grid, block, pl.lds, stream, a);
}

static int32_t enqueue_shared(const ScopedCall &c, int P, const ScopedBuffers &sb, const SearchOut &out, hipStream_t stream) {
    // the slabs' arrival counters; then the slab table
    launch_scoped_prep(c, sb, c.max_slabs, stream);
    shared_slabs_kernel<<<dim3(1), dim3(kScopedThreads), 0, stream>>>(c.group_ptr, c.n_groups, c.plan.qs, c.max_slabs, sb.slabs, sb.n_slabs);
    MIR_HIP(hipGetLastError());
    SharedArgs sa{scoped_args(c, sb, out), c.group_ptr, sb.slabs, sb.n_slabs};
    const dim3 grid((unsigned)c.max_slabs, (unsigned)P);
    for (int round = 0; round * kExactRound < c.k; ++round) {
        sa.s.round = round;
        const int32_t rc = c.ix->dtype == MIR_DTYPE_F16 ? launch_shared<_Float16>(sa, c.plan, grid, stream) : launch_shared<float>(sa, c.plan, grid, stream);
        if (rc != MIR_OK) return rc;
    }
    return MIR_OK;
}

// Device, split, workspace, launches: a device form's on the caller's arrays and stream; a host form's on the workspace's copies, which
// go in as ONE copy of the span carved in the order [q | group_ptr | scope_ptr | seg_begin | seg_end or table | fan-out table] (host_round_trip)
static int32_t run_scoped(const ScopedCall &c) {
    mir_index *ix = c.ix;
    const int32_t rc = use_device(ix->device, nullptr);
    if (rc != MIR_OK) return rc;
    const bool shared = c.n_groups >= 0;
    const int n_scopes = shared ? c.n_groups : c.b;
    const int P = shared ? shared_split(ix->num_cus, c.max_slabs, c.rows.max_rows, kSharedMaxP) : scoped_split(ix->num_cus, c.b, c.rows.max_rows, kScopedMaxP);
    const size_t nseg = c.rows.nseg;
    const ScopedShape shape{c.b, c.k, ix->d, P, nseg, c.host_api, c.blocks, c.n_groups, c.max_slabs, c.expanded};
    ScopedBuffers sb;
    SearchOut stored{};  // the expanded search: the stream kernel's lists of stored rows, in the workspace
    auto enqueue = [&](const ScopedCall &on_device, const SearchOut &out, hipStream_t s) -> int32_t {
        if (shared) return enqueue_shared(on_device, P, sb, out, s);
        if (!c.expanded) return enqueue_scoped(on_device, P, sb, out, s);
        const int32_t rc2 = enqueue_scoped(on_device, P, sb, stored, s);
        if (rc2 != MIR_OK) return rc2;
        const ExpandArgs ea{on_device.table, on_device.fan_table, c.k, stored.doc, stored.row, stored.dist, stored.count,
                            out.doc, out.chunk, out.row, out.dist, out.count, out.flags};
        expand_topk_kernel<<<dim3((unsigned)c.b), dim3(kExpandThreads), 0, s>>>(ea, ExpandFlatScope{on_device.scope_ptr});
        MIR_HIP(hipGetLastError());
        return MIR_OK;
    };
    return with_workspace(
        ix, c.stream, c.host_api,
        [&](char *base) { return c.expanded ? carve_expanded(sb, stored, base, shape, kExactRound) : carve_scoped(sb, base, shape, kExactRound); },
        [&](Workspace *w, hipStream_t s) {
            if (!c.host_api) return enqueue(c, c.out, s);
            HostPiece in[6];
            int n = 0;
            in[n++] = {sb.q, c.queries, (size_t)c.b * ix->d * sizeof(double)};
            if (shared) in[n++] = {sb.group_ptr, c.group_ptr, ((size_t)n_scopes + 1) * 4};
            in[n++] = {sb.scope_ptr, c.scope_ptr, ((size_t)n_scopes + 1) * 4};
            if (nseg) in[n++] = c.blocks ? HostPiece{sb.table, c.table, nseg * sizeof(mir_block_desc)} : HostPiece{sb.seg_begin, c.seg_begin, nseg * 8};
            if (nseg && !c.blocks) in[n++] = {sb.seg_end, c.seg_end, nseg * 8};
            if (nseg && c.expanded) in[n++] = {sb.fan_table, c.fan_table, nseg * sizeof(mir_fanout_desc)};
            ScopedCall dev = c;  // the call as the kernels see it
            dev.queries = sb.q; dev.group_ptr = sb.group_ptr; dev.scope_ptr = sb.scope_ptr;
            dev.seg_begin = sb.seg_begin; dev.seg_end = sb.seg_end; dev.table = sb.table; dev.fan_table = sb.fan_table;
            return host_round_trip(w, s, in, n, sb.q, sb.in_span, sb.out, c.out, c.b, c.k, [&](const SearchOut &out) { return enqueue(dev, out, s); });
        });
}

}  // namespace mir

extern "C" {

int32_t mir_index_search_scoped_device(mir_index *idx, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                       const int32_t *scope_ptr_device, const int64_t *seg_begin_device,
                                       const int64_t *seg_end_device, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row,
                                       double *out_dist, int32_t *out_count, int32_t *out_flags, void *stream_) {
    int32_t rc = check_scoped_args(idx, queries_device, b, k, metric, scope_ptr_device, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    ScopedCall c{idx, queries_device, b, k, metric, scope_ptr_device, seg_begin_device, seg_end_device, nullptr, false,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}, static_cast<hipStream_t>(stream_)};
    return run_scoped(c);
}

int32_t mir_index_search_scoped(mir_index *idx, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                const int32_t *scope_ptr_host, const int64_t *seg_begin_host, const int64_t *seg_end_host,
                                int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                int32_t *out_flags) {
    int32_t rc = check_scoped_args(idx, queries_host, b, k, metric, scope_ptr_host, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    // everything the device form leaves to the kernel's clamping is refused here, before anything is launched
    rc = check_ptr_array(scope_ptr_host, b, "scope_ptr", "query");
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(scope_ptr_host[b] == 0 || (seg_begin_host != nullptr && seg_end_host != nullptr), "segment arrays are NULL");
    ScopedCall c{idx, queries_host, b, k, metric, scope_ptr_host, seg_begin_host, seg_end_host, nullptr, false,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}};
    c.host_api = true;
    rc = walk_scopes(scope_ptr_host, b, "query", nullptr, range_rows(seg_begin_host, seg_end_host, idx->n), &c.rows);
    return rc != MIR_OK ? rc : run_scoped(c);
}

// ---- block search: the scoped search over row blocks (a mir_blocks searcher holds no rows)

int32_t mir_blocks_create(int32_t d, int32_t dtype, int32_t device, mir_blocks **out) {
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    mir_index *dummy = nullptr;
    int32_t rc = check_create_args(0, d, dtype, &dummy);
    if (rc != MIR_OK) return rc;
    int cus = 0;
    rc = use_device(device, &cus);
    if (rc != MIR_OK) return rc;
    mir_blocks *s = new (std::nothrow) mir_blocks();
    mir_index *ix = new (std::nothrow) mir_index();
    if (!s || !ix) {
        delete s;
        delete ix;
        set_error("out of host memory");
        return MIR_ERR_INVALID;
    }
    ix->device = device; ix->num_cus = cus; ix->d = d; ix->dtype = dtype;
    s->ix = ix;
    *out = s;
    return MIR_OK;
}

int32_t mir_blocks_destroy(mir_blocks *s) {
    if (!s) return MIR_OK;
    free_index(s->ix);
    delete s;
    return MIR_OK;
}

int32_t mir_blocks_search_device(mir_blocks *s_, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                 const int32_t *scope_ptr_device, const mir_block_desc *table_device, int32_t *out_doc,
                                 int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags,
                                 void *stream_) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_device, b, k, metric, scope_ptr_device, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    ScopedCall c{s_->ix, queries_device, b, k, metric, scope_ptr_device, nullptr, nullptr, table_device, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}, static_cast<hipStream_t>(stream_)};
    return run_scoped(c);
}

int32_t mir_blocks_search(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                          const int32_t *scope_ptr_host, const mir_rows *const *blocks_host, int32_t *out_doc, int64_t *out_chunk,
                          int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_host, b, k, metric, scope_ptr_host, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    std::vector<mir_block_desc> table;
    ScopedCall c{s_->ix, queries_host, b, k, metric, scope_ptr_host, nullptr, nullptr, nullptr, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}};
    rc = check_blocks(s_->ix, scope_ptr_host, b, "query", nullptr, blocks_host, table, &c.rows);
    if (rc != MIR_OK) return rc;
    c.host_api = true; c.table = table.data();
    return run_scoped(c);
}

// ---- expanded block search: rows stored once, hits expanded to the rows they stand for (vec_fanout_layout.h, vec_kernels_expand.h)

int32_t mir_fanout_create(int64_t n_rows, const int64_t *rep_ptr_host, const int64_t *rep_chunk_host, const int64_t *rep_pos_host,
                          int32_t device, mir_fanout **out) {
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    int32_t rc = check_fanout(n_rows, rep_ptr_host, rep_chunk_host, rep_pos_host);
    if (rc != MIR_OK) return rc;
    rc = use_device(device, nullptr);
    if (rc != MIR_OK) return rc;
    mir_fanout *f = new (std::nothrow) mir_fanout();
    MIR_REQUIRE(f != nullptr, "out of host memory");
    f->device = device; f->n = n_rows; f->R = rep_ptr_host[n_rows];
    const size_t pb = ((size_t)n_rows + 1) * 8, rb = (size_t)f->R * 8;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&f->d_ptr), pb);
    if (e == hipSuccess) e = hipMemcpy(f->d_ptr, rep_ptr_host, pb, hipMemcpyHostToDevice);
    if (f->R > 0) {
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->d_chunk), rb);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->d_pos), rb);
        if (e == hipSuccess) e = hipMemcpy(f->d_chunk, rep_chunk_host, rb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(f->d_pos, rep_pos_host, rb, hipMemcpyHostToDevice);
    }
    f->hbm_bytes = (int64_t)(pb + 2 * rb);
    if (e != hipSuccess) {
        set_error("mir_fanout_create: %s", hipGetErrorString(e));
        mir_fanout_destroy(f);
        return MIR_ERR_HIP;
    }
    *out = f;
    return MIR_OK;
}

int32_t mir_fanout_info(const mir_fanout *f, int64_t *n_rows, int64_t *n_replicas, int32_t *device, int64_t *hbm_bytes) {
    MIR_REQUIRE(f != nullptr, "handle is NULL");
    if (n_rows) *n_rows = f->n;
    if (n_replicas) *n_replicas = f->R;
    if (device) *device = f->device;
    if (hbm_bytes) *hbm_bytes = f->hbm_bytes;
    return MIR_OK;
}

int32_t mir_fanout_get_desc(const mir_fanout *f, mir_fanout_desc *out) {
    MIR_REQUIRE(f != nullptr, "handle is NULL");
    MIR_REQUIRE(out != nullptr, "out is NULL");
    *out = mir_fanout_desc{f->d_ptr, f->d_chunk, f->d_pos, f->n};
    return MIR_OK;
}

int32_t mir_fanout_destroy(mir_fanout *f) {
    if (!f) return MIR_OK;
    (void)hipSetDevice(f->device);
    (void)hipFree(f->d_ptr);
    (void)hipFree(f->d_chunk);
    (void)hipFree(f->d_pos);
    delete f;
    return MIR_OK;
}

int32_t mir_blocks_search_expanded_device(mir_blocks *s_, const double *queries_device, int32_t b, int32_t k, int32_t metric,
                                          const int32_t *scope_ptr_device, const mir_block_desc *table_device,
                                          const mir_fanout_desc *fanout_table_device, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row,
                                          double *out_dist, int32_t *out_count, int32_t *out_flags, void *stream_) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_device, b, k, metric, scope_ptr_device, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    ScopedCall c{s_->ix, queries_device, b, k, metric, scope_ptr_device, nullptr, nullptr, table_device, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}, static_cast<hipStream_t>(stream_)};
    c.expanded = true; c.fan_table = fanout_table_device;
    return run_scoped(c);
}

int32_t mir_blocks_search_expanded(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric,
                                   const int32_t *scope_ptr_host, const mir_rows *const *blocks_host, const mir_fanout *const *fanouts_host,
                                   int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                   int32_t *out_flags) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_host, b, k, metric, scope_ptr_host, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    std::vector<mir_block_desc> table;
    ScopedCall c{s_->ix, queries_host, b, k, metric, scope_ptr_host, nullptr, nullptr, nullptr, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}};
    rc = check_blocks(s_->ix, scope_ptr_host, b, "query", nullptr, blocks_host, table, &c.rows);
    if (rc != MIR_OK) return rc;
    std::vector<mir_fanout_desc> fan_table;
    rc = mir::check_fanouts(scope_ptr_host, b, blocks_host, fanouts_host, table.size(), &fan_table);
    if (rc != MIR_OK) return rc;
    c.host_api = true; c.table = table.data();
    c.expanded = true; c.fan_table = fan_table.data();
    return run_scoped(c);
}

// ---- shared block search: the queries of a group search one scope, whose rows are read once per slab (vec_kernels_shared.h)

int32_t mir_blocks_search_shared_device(mir_blocks *s_, const double *queries_device, int32_t b, int32_t k, int32_t metric, int32_t n_groups,
                                        const int32_t *group_ptr_device, const int32_t *scope_ptr_device, const mir_block_desc *table_device,
                                        int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                        int32_t *out_flags, void *stream_) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_device, b, k, metric, scope_ptr_device, out_count);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(n_groups >= 0, "n_groups=%d is negative", n_groups);
    if (b == 0) return MIR_OK;
    MIR_REQUIRE(group_ptr_device != nullptr, "group_ptr is NULL");
    ScopedCall c{s_->ix, queries_device, b, k, metric, scope_ptr_device, nullptr, nullptr, table_device, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}, static_cast<hipStream_t>(stream_)};
    c.n_groups = n_groups; c.group_ptr = group_ptr_device;
    c.plan = shared_plan(s_->ix->d, k, kExactRound, kScopedWaves);
    c.max_slabs = shared_max_slabs(b, n_groups, c.plan.qs);
    return run_scoped(c);
}

int32_t mir_blocks_search_shared(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, int32_t n_groups,
                                 const int32_t *group_ptr_host, const int32_t *scope_ptr_host, const mir_rows *const *blocks_host,
                                 int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count,
                                 int32_t *out_flags) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    int32_t rc = check_scoped_args(s_->ix, queries_host, b, k, metric, scope_ptr_host, out_count);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(n_groups >= 0, "n_groups=%d is negative", n_groups);
    if (b == 0) return MIR_OK;
    // everything the device form trusts is checked here, before anything is launched
    MIR_REQUIRE(group_ptr_host != nullptr, "group_ptr is NULL");
    rc = check_ptr_array(group_ptr_host, n_groups, "group_ptr", "group");
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(group_ptr_host[n_groups] == b, "group_ptr[n_groups]=%d must be b=%d", group_ptr_host[n_groups], b);
    std::vector<mir_block_desc> table;
    ScopedCall c{s_->ix, queries_host, b, k, metric, scope_ptr_host, nullptr, nullptr, nullptr, true,
                 {out_doc, out_chunk, out_row, out_dist, out_count, out_flags}};
    rc = check_blocks(s_->ix, scope_ptr_host, n_groups, "group", group_ptr_host, blocks_host, table, &c.rows);
    if (rc != MIR_OK) return rc;
    c.host_api = true; c.table = table.data();
    c.n_groups = n_groups; c.group_ptr = group_ptr_host;
    c.plan = shared_plan(s_->ix->d, k, kExactRound, kScopedWaves);
    c.max_slabs = shared_slab_count(group_ptr_host, n_groups, c.plan.qs);  // (no surplus workgroup, as the device form's bound leaves)
    return run_scoped(c);
}

// ---- pieces search: scopes that overlap read their common blocks once (vec_pieces_layout.h, vec_kernels_pieces.h)

// The three pieces entries' one host path.  piece_index: NULL, or per piece NULL / the index composed of that piece's rows.
// fanouts: NULL, or per entry of blocks_host NULL / that block's fan-out; where one is given the merge leaves the stored rows'
// lists in the workspace and expand_topk_kernel<ExpandPiecesScope> writes the answer (vec_pieces_expanded_layout.h)
static int32_t run_pieces(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, int32_t n_pieces,
                          const int32_t *piece_ptr_host, const mir_rows *const *blocks_host, const int32_t *rider_ptr_host,
                          const int32_t *rider_piece_host, int32_t min_riders, const mir_index *const *piece_index,
                          const mir_fanout *const *fanouts, const SearchOut &user) {
    MIR_REQUIRE(s_ != nullptr, "searcher is NULL");
    mir_index *ix = s_->ix;
    int32_t rc = check_search_args(ix, queries_host, b, k, metric, user.count);
    if (rc != MIR_OK) return rc;
    MIR_REQUIRE(n_pieces >= 0, "n_pieces=%d is negative", n_pieces);
    MIR_REQUIRE(min_riders >= 1, "min_riders=%d must be >= 1", min_riders);
    if (b == 0) return MIR_OK;
    // everything the kernels trust is checked here, before anything is launched
    rc = check_pieces_args(b, n_pieces, piece_ptr_host, rider_ptr_host, rider_piece_host, min_riders);
    if (rc != MIR_OK) return rc;
    std::vector<mir_block_desc> all;  // one descriptor per entry of blocks_host
    ScopeRows piece_rows{0, 0};
    if (n_pieces > 0) {
        rc = check_blocks(ix, piece_ptr_host, n_pieces, "piece", nullptr, blocks_host, all, &piece_rows);
        if (rc != MIR_OK) return rc;
    }
    auto index_of = [&](int p) { return piece_index ? const_cast<mir_index *>(piece_index[p]) : nullptr; };
    for (int p = 0; p < n_pieces; ++p) {
        const mir_index *px = index_of(p);
        if (!px) continue;
        MIR_REQUIRE(px->d == ix->d && px->dtype == ix->dtype && px->device == ix->device,
                    "the index of piece %d is %d-dimensional dtype %d on device %d, the searcher %d-dimensional dtype %d on device %d", p,
                    px->d, px->dtype, px->device, ix->d, ix->dtype, ix->device);
        MIR_REQUIRE(px->row_offset == 0, "the index of piece %d has row_offset %lld: must be 0", p, (long long)px->row_offset);
        MIR_REQUIRE(px->n > 0, "the index of piece %d holds no row", p);
        int64_t rows = 0;
        for (int t = piece_ptr_host[p]; t < piece_ptr_host[p + 1]; ++t) rows += all[(size_t)t].n;
        MIR_REQUIRE(px->n == rows, "the index of piece %d holds %lld rows, its blocks %lld", p, (long long)px->n, (long long)rows);
    }
    IndexedPlan ip;
    rc = plan_pieces_indexed(b, n_pieces, piece_ptr_host, rider_ptr_host, rider_piece_host, min_riders, [&](int p) { return index_of(p) != nullptr; },
                             [&](int t) { return (uint64_t)all[(size_t)t].n; }, &ip);
    if (rc != MIR_OK) return rc;
    // the fan-outs against their blocks, while they become the descriptor table the expansion reads; the expanded scopes' rows
    const size_t n_blocks = all.size();
    std::vector<mir_fanout_desc> fan_table;
    ExpandedPiecesPlan ep;
    ExpandedPiecesShape eshape;
    for (size_t t = 0; fanouts && t < n_blocks && !eshape.on; ++t) eshape.on = fanouts[t] != nullptr;
    if (eshape.on) {
        fan_table.assign(n_blocks, mir_fanout_desc{nullptr, nullptr, nullptr, 0});
        for (int p = 0; p < n_pieces; ++p)
            for (int t = piece_ptr_host[p]; t < piece_ptr_host[p + 1]; ++t) {
                const mir_fanout *f = fanouts[t];
                if (!f) continue;
                MIR_REQUIRE(f->n == blocks_host[t]->n && f->device == blocks_host[t]->device,
                            "the fan-out of block %d of piece %d is of %lld stored rows on device %d, the block holds %lld on device %d",
                            t - piece_ptr_host[p], p, (long long)f->n, f->device, (long long)blocks_host[t]->n, blocks_host[t]->device);
                fan_table[(size_t)t] = mir_fanout_desc{f->d_ptr, f->d_chunk, f->d_pos, f->n};
            }
        rc = plan_pieces_expanded(b, n_pieces, piece_ptr_host, rider_ptr_host, rider_piece_host,
                                  [&](int t) { return (uint64_t)(fanouts[t] ? fanouts[t]->R : all[(size_t)t].n); }, &ep);
        if (rc != MIR_OK) return rc;
        eshape.n_blocks = n_blocks; eshape.n_riders = (size_t)rider_ptr_host[b]; eshape.n_pieces = n_pieces;
    }
    const PiecesPlan &pl = ip.pl;
    const int n_occ = pl.n_occ(), n_groups = pl.n_groups(), d = ix->d;
    const int gs = ip.n_shared_groups(), n_shared = ip.n_shared_occ();  // what the shared search sees: the index groups and their rides lie behind
    MIR_REQUIRE((int64_t)n_occ * k < (1ll << 31), "%d occurrences of k=%d results are 2^31 list entries or more", n_occ, k);
    const size_t nseg_shared = pl.shared_block.size(), nseg_solo = pl.solo_block.size();
    std::vector<mir_block_desc> table(nseg_shared + nseg_solo);  // the groups' blocks, then the solo occurrences'
    for (size_t i = 0; i < nseg_shared; ++i) table[i] = all[(size_t)pl.shared_block[i]];
    for (size_t i = 0; i < nseg_solo; ++i) table[nseg_shared + i] = all[(size_t)pl.solo_block[i]];
    rc = use_device(ix->device, nullptr);
    if (rc != MIR_OK) return rc;
    const SharedPlan plan = shared_plan(d, k, kExactRound, kScopedWaves);
    const int max_slabs = shared_slab_count(pl.group_ptr.data(), gs, plan.qs);
    const int P_shared = shared_split(ix->num_cus, max_slabs, pl.shared_max_rows, kSharedMaxP);
    const int P_solo = scoped_split(ix->num_cus, pl.n_solo, pl.solo_max_rows, kScopedMaxP);
    const PiecesShape shape{b, k, d, pl.n_shared, pl.n_solo, n_groups, nseg_shared, nseg_solo, P_shared, P_solo, max_slabs};
    const IndexedShape xshape{ip.n_index_groups, ip.n_index_occ, ip.prefix.size()};
    PiecesBuffers pb;
    IndexedBuffers xb;
    ExpandedPiecesBuffers eb;
    return with_workspace(
        ix, nullptr, true, [&](char *base) { return carve_pieces_expanded(pb, xb, eb, base, shape, xshape, eshape, kExactRound); },
        [&](Workspace *w, hipStream_t s) {
            HostPiece in[18];
            int n = 0;
            auto piece = [&](const void *dev, const void *host, size_t bytes) {
                if (bytes) in[n++] = {dev, host, bytes};
            };
            piece(pb.q, queries_host, (size_t)b * d * sizeof(double));
            piece(pb.occ_query, pl.occ_query.data(), (size_t)n_occ * 4);
            piece(pb.group_ptr, pl.group_ptr.data(), ((size_t)n_groups + 1) * 4);
            piece(pb.scope_ptr, pl.scope_ptr.data(), ((size_t)n_groups + 1) * 4);
            piece(pb.solo_ptr, pl.solo_ptr.data(), ((size_t)pl.n_solo + 1) * 4);
            piece(pb.table, table.data(), table.size() * sizeof(mir_block_desc));
            piece(pb.occ_base, pl.occ_base.data(), (size_t)pl.n_shared * 4);
            piece(pb.solo_ord, pl.solo_ord.data(), nseg_solo * 4);
            piece(pb.q_occ_ptr, pl.q_occ_ptr.data(), ((size_t)b + 1) * 4);
            piece(pb.q_occ, pl.q_occ.data(), (size_t)n_occ * 4);
            piece(xb.prefix, ip.prefix.data(), ip.prefix.size() * 8);
            if (eshape.on) {
                piece(eb.all_table, all.data(), n_blocks * sizeof(mir_block_desc));
                piece(eb.fan_table, fan_table.data(), n_blocks * sizeof(mir_fanout_desc));
                piece(eb.piece_ptr, piece_ptr_host, ((size_t)n_pieces + 1) * 4);
                piece(eb.rider_ptr, rider_ptr_host, ((size_t)b + 1) * 4);
                piece(eb.rider_piece, rider_piece_host, eshape.n_riders * 4);
                piece(eb.rider_base, ep.rider_base.data(), eshape.n_riders * 4);
                piece(eb.piece_rows, ep.piece_rows.data(), (size_t)n_pieces * 8);
            }
            return host_round_trip(w, s, in, n, pb.q, pb.in_span, pb.out, user, b, k, [&](const SearchOut &out) -> int32_t {
                if (n_occ > 0) pieces_gather_kernel<<<dim3((unsigned)n_occ), dim3(64), 0, s>>>(pb.q, pb.occ_query, b, d, pb.q_by_occ);
                MIR_HIP(hipGetLastError());
                const size_t sk = (size_t)pl.n_shared * k;  // the solo occurrences' results lie behind the shared and the index ones'
                if (n_shared > 0) {
                    ScopedCall c{ix, pb.q_by_occ, n_shared, k, metric, pb.scope_ptr, nullptr, nullptr, pb.table, true, SearchOut{}};
                    c.n_groups = gs; c.group_ptr = pb.group_ptr; c.plan = plan; c.max_slabs = max_slabs;
                    const int32_t rc2 = enqueue_shared(c, P_shared, pb.shared, pb.occ, s);
                    if (rc2 != MIR_OK) return rc2;
                }
                if (pl.n_solo > 0) {
                    ScopedCall c{ix, pb.q_by_occ + (size_t)pl.n_shared * d, pl.n_solo, k, metric, pb.solo_ptr, nullptr, nullptr, pb.table + nseg_shared, true, SearchOut{}};
                    const SearchOut occ{pb.occ.doc + sk, pb.occ.chunk + sk, pb.occ.row + sk, pb.occ.dist + sk, pb.occ.count + pl.n_shared, pb.occ.flags + pl.n_shared};
                    const int32_t rc2 = enqueue_scoped(c, P_solo, pb.solo, occ, s);
                    if (rc2 != MIR_OK) return rc2;
                }
                if (ip.n_index_occ > 0) {  // the gathered queries' norms, for the rescore kernel
                    prep_queries_kernel<<<dim3((unsigned)ip.n_index_occ), dim3(64), 0, s>>>(pb.q_by_occ + (size_t)n_shared * d, ip.n_index_occ, d, 0, 0, nullptr,
                                                                                             xb.q_sq, xb.q_norm, nullptr, 0);
                    MIR_HIP(hipGetLastError());
                }
                for (int gx = 0; gx < ip.n_index_groups; ++gx) {
                    // One batched search of the piece's index over its rides, on this call's stream: the index takes a workspace
                    // of its own and gives it back pending on `s` (mir_index_search_device); no mutex of either handle is held here.
                    const int g = gs + gx, o0 = pl.group_ptr[(size_t)g], nq = pl.group_ptr[(size_t)g + 1] - o0;
                    const size_t r0 = (size_t)o0 * k;
                    const int32_t rc2 = mir_index_search_device(index_of(pl.group_piece[(size_t)g]), pb.q_by_occ + (size_t)o0 * d, nq, k, metric, pb.occ.doc + r0,
                                                                pb.occ.chunk + r0, pb.occ.row + r0, pb.occ.dist + r0, pb.occ.count + o0, pb.occ.flags + o0, s);
                    if (rc2 != MIR_OK) return rc2;
                    const int t0 = pl.scope_ptr[(size_t)g], x0 = o0 - n_shared;
                    const PiecesRescoreArgs ra{pb.q_by_occ + (size_t)o0 * d, xb.q_sq + x0, xb.q_norm + x0, pb.table + t0, xb.prefix + ip.prefix_ptr[(size_t)gx],
                                               pl.scope_ptr[(size_t)g + 1] - t0, d, metric, k, pb.occ.count + o0, pb.occ.doc + r0, pb.occ.chunk + r0,
                                               pb.occ.row + r0, pb.occ.dist + r0};
                    if (ix->dtype == MIR_DTYPE_F16) pieces_rescore_kernel<_Float16><<<dim3((unsigned)nq), dim3(kPiecesThreads), 0, s>>>(ra);
                    else pieces_rescore_kernel<float><<<dim3((unsigned)nq), dim3(kPiecesThreads), 0, s>>>(ra);
                    MIR_HIP(hipGetLastError());
                }
                const PiecesMergeArgs ma{pb.q_occ_ptr, pb.q_occ, pl.n_shared, pl.n_solo, pb.occ_base, pb.solo_ptr, pb.solo_ord, k, pb.occ,
                                         pb.cand_key, pb.cand_row, pb.cand_src, eshape.on ? eb.stored : out};
                pieces_merge_kernel<<<dim3((unsigned)b), dim3(kPiecesThreads), 0, s>>>(ma);
                MIR_HIP(hipGetLastError());
                if (eshape.on) {  // the stored rows' lists -> the first k rows of the expanded flattened scopes
                    const ExpandArgs ea{eb.all_table, eb.fan_table, k, eb.stored.doc, eb.stored.row, eb.stored.dist, eb.stored.count,
                                        out.doc, out.chunk, out.row, out.dist, out.count, out.flags};
                    const ExpandPiecesScope scope{PiecesScopes{eb.piece_ptr, eb.rider_ptr, eb.rider_piece, eb.rider_base, eb.piece_rows, n_pieces,
                                                               (int32_t)eshape.n_riders, (int32_t)n_blocks}};
                    expand_topk_kernel<<<dim3((unsigned)b), dim3(kExpandThreads), 0, s>>>(ea, scope);
                    MIR_HIP(hipGetLastError());
                }
                return MIR_OK;
            });
        });
}

int32_t mir_blocks_search_pieces(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, int32_t n_pieces,
                                 const int32_t *piece_ptr_host, const mir_rows *const *blocks_host, const int32_t *rider_ptr_host,
                                 const int32_t *rider_piece_host, int32_t min_riders, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row,
                                 double *out_dist, int32_t *out_count, int32_t *out_flags) {
    return run_pieces(s_, queries_host, b, k, metric, n_pieces, piece_ptr_host, blocks_host, rider_ptr_host, rider_piece_host, min_riders, nullptr,
                      nullptr, SearchOut{out_doc, out_chunk, out_row, out_dist, out_count, out_flags});
}

// ---- the same with frozen runs: a piece that comes with an index is searched through it (vec_frozen_layout.h)

int32_t mir_blocks_search_pieces_indexed(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, int32_t n_pieces,
                                         const int32_t *piece_ptr_host, const mir_rows *const *blocks_host, const mir_index *const *piece_index_host,
                                         const int32_t *rider_ptr_host, const int32_t *rider_piece_host, int32_t min_riders, int32_t *out_doc,
                                         int64_t *out_chunk, int64_t *out_row, double *out_dist, int32_t *out_count, int32_t *out_flags) {
    return run_pieces(s_, queries_host, b, k, metric, n_pieces, piece_ptr_host, blocks_host, rider_ptr_host, rider_piece_host, min_riders, piece_index_host,
                      nullptr, SearchOut{out_doc, out_chunk, out_row, out_dist, out_count, out_flags});
}

// ---- the same over paged blocks: the routes select stored rows, the hits are expanded on device (vec_pieces_expanded_layout.h)

int32_t mir_blocks_search_pieces_expanded(mir_blocks *s_, const double *queries_host, int32_t b, int32_t k, int32_t metric, int32_t n_pieces,
                                          const int32_t *piece_ptr_host, const mir_rows *const *blocks_host, const mir_fanout *const *fanouts_host,
                                          const mir_index *const *piece_index_host, const int32_t *rider_ptr_host, const int32_t *rider_piece_host,
                                          int32_t min_riders, int32_t *out_doc, int64_t *out_chunk, int64_t *out_row, double *out_dist,
                                          int32_t *out_count, int32_t *out_flags) {
    return run_pieces(s_, queries_host, b, k, metric, n_pieces, piece_ptr_host, blocks_host, rider_ptr_host, rider_piece_host, min_riders, piece_index_host,
                      fanouts_host, SearchOut{out_doc, out_chunk, out_row, out_dist, out_count, out_flags});
}

int32_t mir_index_metric_eval(mir_index *idx, const double *query_host, int32_t metric, double *out_host) {
    MIR_REQUIRE(idx != nullptr, "index is NULL");
    MIR_REQUIRE(metric >= 0 && metric <= 3, "unknown metric %d", metric);
    if (idx->n == 0) return MIR_OK;
    MIR_REQUIRE(query_host != nullptr && out_host != nullptr, "NULL buffer");
    int32_t rc = use_device(idx->device, nullptr);
    if (rc != MIR_OK) return rc;
    const int d = idx->d;
    const int64_t n = idx->n;
    double *dq = nullptr, *dsq = nullptr, *dnm = nullptr, *dout = nullptr;
    return with_workspace(
        idx, nullptr, true,
        [&](char *base) {  // slab: q[d] | q_sq | q_norm | out[n]
            Carver c{base};
            dq = c.take<double>(d);
            dsq = c.take<double>(1);
            dnm = c.take<double>(1);
            dout = c.take<double>(n);
            return c.off + 256;
        },
        [&](Workspace *, hipStream_t s) {
            hipError_t e = hipMemcpyAsync(dq, query_host, (size_t)d * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) {
                // ngroups = 0: only the per-query norm block runs
                prep_queries_kernel<<<dim3(1), dim3(64), 0, s>>>(dq, 1, d, idx->ksteps, 0, nullptr, dsq, dnm, nullptr, 0);
                if (idx->native16)
                    metric_eval_kernel<_Float16><<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(idx->d_f16, idx->d_docsq, n, d,
                                                                                                    dq, dsq, dnm, metric, dout);
                else
                    metric_eval_kernel<float><<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(idx->d_orig, idx->d_docsq, n, d, dq,
                                                                                                 dsq, dnm, metric, dout);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(out_host, dout, (size_t)n * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            else (void)hipStreamSynchronize(s);
            if (e != hipSuccess) {
                set_error("metric_eval failed: %s", hipGetErrorString(e));
                return (int32_t)MIR_ERR_HIP;
            }
            return (int32_t)MIR_OK;
        });
}

int32_t mir_metric_eval(const void *docs_host, int64_t n, int32_t d, int32_t dtype, const double *query_host,
                        int32_t metric, int32_t device, double *out_host) {
    mir_index *ix = nullptr;
    int32_t rc = mir_index_create(docs_host, n, d, dtype, nullptr, nullptr, device, 0, &ix);
    if (rc != MIR_OK) return rc;
    rc = mir_index_metric_eval(ix, query_host, metric, out_host);
    mir_index_destroy(ix);
    return rc;
}

// The merge entries' arguments; b = 0 merges nothing and needs no buffers
static int32_t check_merge_args(const double *dist, const int64_t *row, const int32_t *count, int32_t s, int64_t shard_stride_bytes,
                                int32_t b, int32_t k, const double *out_dist, const int64_t *out_row, const int32_t *out_count) {
    MIR_REQUIRE(s >= 1 && b >= 0 && k >= 1, "bad merge shape s=%d b=%d k=%d", s, b, k);
    MIR_REQUIRE(shard_stride_bytes >= 0 && shard_stride_bytes % 8 == 0, "shard stride must be a multiple of 8");
    MIR_REQUIRE(b == 0 || (dist && row && count && out_dist && out_row && out_count), "NULL buffer");
    return MIR_OK;
}

// bytes from one shard's array to the next: the caller's stride, or (0) dense [s][b][k] / [s][b] arrays
struct MergeStrides {
    int64_t dist, row, count;
};
static MergeStrides merge_strides(int64_t shard_stride_bytes, int32_t b, int32_t k) {
    if (shard_stride_bytes) return {shard_stride_bytes, shard_stride_bytes, shard_stride_bytes};
    return {(int64_t)b * k * 8, (int64_t)b * k * 8, (int64_t)b * 4};
}

int32_t mir_topk_merge_device(const double *dist, const int64_t *row, const int32_t *count, int32_t s,
                              int64_t shard_stride_bytes, int32_t b, int32_t k, int32_t descending_scores,
                              double *out_dist, int64_t *out_row, int32_t *out_count, int32_t device,
                              void *stream) {
    int32_t rc = check_merge_args(dist, row, count, s, shard_stride_bytes, b, k, out_dist, out_row, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    rc = use_device(device, nullptr);
    if (rc != MIR_OK) return rc;
    const MergeStrides st = merge_strides(shard_stride_bytes, b, k);
    const int64_t nk = (int64_t)s * k;
    if (nk <= kMergeLds)
        merge_topk_kernel<<<dim3(b), dim3(nk <= 64 ? 64 : nk <= 128 ? 128 : 256), 0, static_cast<hipStream_t>(stream)>>>(
            reinterpret_cast<const char *>(dist), reinterpret_cast<const char *>(row),
            reinterpret_cast<const char *>(count), s, st.dist, st.row, st.count, b, k, descending_scores, out_dist, out_row, out_count);
    else
        merge_topk_global_kernel<<<dim3(b), dim3(64), 0, static_cast<hipStream_t>(stream)>>>(
            reinterpret_cast<const char *>(dist), reinterpret_cast<const char *>(row),
            reinterpret_cast<const char *>(count), s, st.dist, st.row, st.count, b, k, descending_scores, out_dist, out_row, out_count);
    MIR_HIP(hipGetLastError());
    return MIR_OK;
}

int32_t mir_topk_merge_host(const double *dist, const int64_t *row, const int32_t *count, int32_t s,
                            int64_t shard_stride_bytes, int32_t b, int32_t k, int32_t descending_scores,
                            double *out_dist, int64_t *out_row, int32_t *out_count) {
    const int32_t rc = check_merge_args(dist, row, count, s, shard_stride_bytes, b, k, out_dist, out_row, out_count);
    if (rc != MIR_OK || b == 0) return rc;
    const MergeStrides st = merge_strides(shard_stride_bytes, b, k);
    struct Item {
        uint64_t key;  // merge_order.h: the one order of the three merge implementations
        int64_t r;
        double d;
    };
    std::vector<Item> items;
    for (int q = 0; q < b; ++q) {
        items.clear();
        for (int sh = 0; sh < s; ++sh) {
            const int c = reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(count) + sh * st.count)[q];
            MIR_REQUIRE(c >= 0 && c <= k, "count[%d][%d]=%d out of range", sh, q, c);
            const double *dp = reinterpret_cast<const double *>(reinterpret_cast<const char *>(dist) + sh * st.dist);
            const int64_t *rp = reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(row) + sh * st.row);
            for (int p = 0; p < c; ++p) {
                const double d = dp[(size_t)q * k + p];
                items.push_back({mir::merge_order_key(d, descending_scores), rp[(size_t)q * k + p], d});
            }
        }
        std::sort(items.begin(), items.end(), [descending_scores](const Item &a, const Item &c) {
            return mir::merge_before(a.key, a.r, c.key, c.r, descending_scores);
        });
        const int kout = (int)std::min<size_t>(items.size(), (size_t)k);
        for (int p = 0; p < kout; ++p) {
            out_dist[(size_t)q * k + p] = items[p].d;
            out_row[(size_t)q * k + p] = items[p].r;
        }
        out_count[q] = kout;
    }
    return MIR_OK;
}

}  // extern "C"
