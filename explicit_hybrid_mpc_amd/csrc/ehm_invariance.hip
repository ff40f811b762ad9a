// One-step invariance of a compiled law leaf by leaf.  On a leaf the law is
// affine, in the leaf's step-0 mode the plant of rollout_apply is affine in (x, u, d), so the
// successor map (x, d) -> x+ is affine on cell x box and the image of the leaf under every
// disturbance of the box is the convex hull of its successors at the (p + 1) 2^n_d points (cell
// vertex, box corner).  Where the roots' union is convex, a leaf all of whose vertex successors lie
// in it is mapped into it as a whole.
//
//   k_successors   one thread per requested leaf, templated on the law's scalar and on P: the cell
//                  and the leaf's map at its vertices (ehm_cells_dev.h), the region rows of the
//                  leaf's mode at every vertex, the plant step in the order of rollout_apply
//                  (ehm_rollout_dev.h; k_reach of ehm_core.hip holds a copy of the step before the
//                  disturbance: DESIGN.md 3.8i, Kernels, says why it is no shared function), every
//                  successor located as one step of k_compiled_rollout locates its state (the
//                  visibility walk from the leaf's own root, else the serial rule;
//                  ehm_compiled_dev.h) and judged by its weights in that root; the counts by the
//                  LDS counters of ehm_verdict.h
//
// The plant sits in LDS (plant_load) with the box after it.  The cell lives in registers as in
// k_certify_cells; the vertex of a pass is picked out of it by selects, so the body is compiled
// once per (T, P).
// Every operation a result depends on runs under fp contract(off) in a fixed order
// (tests/invariance_cpu.py is the numpy mirror).  The worst leaf and the volumes are taken on the
// host in leaf order, so no result depends on the chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_verdict.h"

#define EHM_INV_BLOCK 64
#define EHM_INV_STATUSES 5
#define EHM_INV_BUDGET (1 << 24)    // doubles of x_next one pass may hold (opts->chunk = 0)

namespace {

enum { INV_INVARIANT = 0, INV_EXITS = 1, INV_MODE_REGION = 2, INV_NO_MODE = 3, INV_NO_CELL = 4 };

struct SuccArgs {
    long long n;
    const int32_t* leaf_ids;        // or nullptr: leaves first .. first + n - 1
    long long first;
    const void* node;               // of the law's scalar, as leaf_rec
    const void* leaf_rec;
    const int32_t* root_entry;
    const double* root_rec;         // [n_roots][side_stride]
    const int32_t* nbr;             // [n_roots][P+1] or nullptr
    const double* root_vertices;    // [n_roots][P+1][P]
    ehm_cert::Parents par;
    const int32_t* leaf_mode;       // [n_leaf]
    int n_u, leaf_stride, side_stride, n_roots;
    int n_d, o_lo, o_hi;            // the box: 2^n_d corners, its bounds at sh + o_lo, sh + o_hi
    double tol_exit;
    double* vertices;               // [n][P+1][P]
    int32_t* status;                // [n]
    double* margin;                 // [n]
    int32_t* worst;                 // [n]
    double* max_violation;          // [n]
    double* x_next;                 // [n][P+1][n_c][P] or nullptr
    int32_t* succ_root;             // [n][P+1][n_c] or nullptr
    int32_t* succ_leaf;             // [n][P+1][n_c] or nullptr
    unsigned long long* counters;   // [EHM_INV_STATUSES]
};

// the plane walk of law_input (ehm_compiled_dev.h) from entry k without the leaf's map
template <int P>
__device__ __forceinline__ int succ_walk(const double* __restrict__ node, int k, const double* z) {
#pragma clang fp contract(off)
    constexpr int NS = P <= 6 ? 8 : 16;
    while (k >= 0) {
        const double* r = node + (size_t)k * NS;
        const long long ch = __double_as_longlong(r[P + 1]);
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) s = s + r[c] * z[c];
        s = s + r[P];
        k = (s >= -EHM_C_EPS) ? (int)(ch & 0xffffffffll) : (int)(ch >> 32);
    }
    return ~k;
}

template <int P>
__device__ __forceinline__ int succ_walk(const float* __restrict__ node, int k, const double* z) {
    float xs[P];
#pragma unroll
    for (int c = 0; c < P; ++c) xs[c] = (float)z[c];
    int visited = 0;
    return walk32<P>(node, k, xs, visited);
}

// a beats b as the smaller margin: the smaller number, a NaN before any number; the earlier stays
// on ties
__device__ __forceinline__ bool margin_beats(double a, double b) {
    return a < b || (a != a && b == b);
}

// Everything of one leaf; returns its status.
template <class T, int P>
__device__ __forceinline__ int leaf_successors(const SuccArgs& A, const DevPlant& PL,
                                               const double* sh, long long q) {
#pragma clang fp contract(off)
    const int32_t l = A.leaf_ids ? A.leaf_ids[q] : (int32_t)(A.first + q);
    const int n_u = A.n_u, n_d = A.n_d, n_c = 1 << n_d;
    const T* node = static_cast<const T*>(A.node);
    double V[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, node, A.root_entry, A.root_vertices, l, V);
    double* vout = A.vertices + (size_t)q * (P + 1) * P;
#pragma unroll
    for (int e = 0; e < (P + 1) * P; ++e) vout[e] = ok ? V[e] : NAN;
    const int m = A.leaf_mode[l];
    const size_t pts = (size_t)q * (P + 1) * n_c;
    if (!ok || m < 0 || m >= PL.n_modes) {
        A.margin[q] = NAN;
        A.worst[q] = -1;
        A.max_violation[q] = NAN;
        for (int e = 0; e < (P + 1) * n_c; ++e) {
            if (A.x_next)
#pragma unroll
                for (int c = 0; c < P; ++c) A.x_next[(pts + e) * P + c] = NAN;
            if (A.succ_root) A.succ_root[pts + e] = -1;
            if (A.succ_leaf) A.succ_leaf[pts + e] = -1;
        }
        return ok ? INV_NO_MODE : INV_NO_CELL;
    }
    // the leaf's own root: where the visibility walk of every successor starts
    ehm_cert::TurnSet turns;
    int32_t root = 0;
    (void)ehm_cert::walk_up(A.par, l, turns, root);
    const T* lr = static_cast<const T*>(A.leaf_rec) + (size_t)l * A.leaf_stride;
    const double* sA = sh + PL.oA + m * P * P;
    const double* sB = sh + PL.oB + m * P * n_u;
    const double* sw = sh + PL.ow + m * P;
    const double* sE = sh + PL.oE;
    const double* sG = sh + PL.oG;
    const double* sg = sh + PL.og;
    const double* lo_d = sh + A.o_lo;
    const double* hi_d = sh + A.o_hi;
    bool in_region = true, all_inside = true;
    double best = 0.0, maxv = -__builtin_inf();
    int best_at = -1;
    for (int i = 0; i <= P; ++i) {
        double v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double t = 0.0;
#pragma unroll
            for (int ii = 0; ii <= P; ++ii) t = ii == i ? V[ii * P + c] : t;
            v[c] = t;
        }
        // the region rows of the leaf's mode: the test of rollout_apply
        for (int r = PL.row0[m]; r < PL.row0[m + 1]; ++r) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + sh[PL.oH + r * P + c] * v[c];
            in_region = in_region && (s <= sh[PL.oh + r] + A.tol_exit);
        }
        double u[EHM_R_MAX_NU];
#pragma unroll
        for (int c = 0; c < EHM_R_MAX_NU; ++c)
            u[c] = c < n_u ? leaf_map_at<P>(lr, n_u, c, v) : 0.0;
        // the successor before the disturbance: rollout_apply's nominal branch
        double y[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + sA[k * P + c] * v[c];
#pragma unroll
            for (int c = 0; c < EHM_R_MAX_NU; ++c)
                if (c < n_u) s = s + sB[k * n_u + c] * u[c];
            y[k] = s + sw[k];
        }
        for (int j = 0; j < n_c; ++j) {
            double z[P];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                double s = y[k];
                for (int b = 0; b < n_d; ++b)
                    s = s + sE[k * n_d + b] * (((j >> b) & 1) ? hi_d[b] : lo_d[b]);
                z[k] = s;
            }
            // the root: the step of k_compiled_rollout, the walk started at the leaf's own root
            double alpha[P], a0;
            int kr = root;
            bool found = false;
            if (A.nbr) {
                int kw = root;
                for (int step = 0; step < EHM_C_STEPS; ++step) {
                    c_weights<P>(A.root_rec + (size_t)kw * A.side_stride, z, alpha, a0);
                    double lo = a0;
                    int at = 0;
#pragma unroll
                    for (int c = 0; c < P; ++c)
                        if (alpha[c] < lo) {
                            lo = alpha[c];
                            at = c + 1;
                        }
                    if (lo > EHM_C_STRICT) {
                        found = true;
                        break;
                    }
                    if (lo >= -EHM_C_STRICT) break;
                    const int k2 = A.nbr[(size_t)kw * (P + 1) + at];
                    if (k2 < 0) break;
                    kw = k2;
                }
                if (found) kr = kw;
            }
            if (!found) {
                kr = A.n_roots - 1;
                for (int r = 0; r + 1 < A.n_roots; ++r)
                    if (c_contains<P>(A.root_rec + (size_t)r * A.side_stride, z)) {
                        kr = r;
                        break;
                    }
                c_weights<P>(A.root_rec + (size_t)kr * A.side_stride, z, alpha, a0);
            }
            bool inside = a0 >= -A.tol_exit;
            double mg = a0;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                inside = inside && (alpha[c] >= -A.tol_exit);
                mg = margin_beats(alpha[c], mg) ? alpha[c] : mg;
            }
            all_inside = all_inside && inside;
            const int at = i * n_c + j;
            if (best_at < 0 || margin_beats(mg, best)) {
                best = mg;
                best_at = at;
            }
            for (int r = 0; r < PL.n_g; ++r) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) s = s + sG[r * P + c] * z[c];
                maxv = fmax(maxv, s - sg[r]);
            }
            if (A.x_next)
#pragma unroll
                for (int c = 0; c < P; ++c) A.x_next[(pts + at) * P + c] = z[c];
            if (A.succ_root) A.succ_root[pts + at] = inside ? kr : -1;
            if (A.succ_leaf)
                A.succ_leaf[pts + at] = inside ? succ_walk<P>(node, A.root_entry[kr], z) : -1;
        }
    }
    A.margin[q] = best;
    A.worst[q] = best_at;
    A.max_violation[q] = maxv;
    return !in_region ? INV_MODE_REGION : all_inside ? INV_INVARIANT : INV_EXITS;
}

template <class T, int P>
__global__ __launch_bounds__(EHM_INV_BLOCK) void k_successors(SuccArgs A, DevPlant PL) {
    // all of the block's LDS is dynamic, so its base stays 16-byte aligned: the plant and the box
    // (PL.total doubles), the status counters after them
    extern __shared__ __attribute__((aligned(16))) double sh[];
    unsigned int* cnt = reinterpret_cast<unsigned int*>(sh + PL.total);
    plant_load(PL, sh);
    ehm_verdict::counters_zero<EHM_INV_BLOCK, EHM_INV_STATUSES>(cnt);
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < A.n) {
        const int s = leaf_successors<T, P>(A, PL, sh, q);
        A.status[q] = s;
        atomicAdd(&cnt[s], 1u);
    }
    __syncthreads();
    ehm_verdict::counters_flush<EHM_INV_BLOCK, EHM_INV_STATUSES>(cnt, A.counters);
}

typedef void (*succ_fn)(SuccArgs, DevPlant);
#define EHM_INV_ALL(T) {&k_successors<T, 1>, &k_successors<T, 2>, &k_successors<T, 3>, \
                        &k_successors<T, 4>, &k_successors<T, 5>, &k_successors<T, 6>, \
                        &k_successors<T, 7>, &k_successors<T, 8>}
const succ_fn k_succ64[EHM_CP] = EHM_INV_ALL(double);
const succ_fn k_succ32[EHM_CP] = EHM_INV_ALL(float);
#undef EHM_INV_ALL

thread_local ehm_err_channel v_err;

// a smaller margin, the earlier leaf on ties; a NaN never wins
bool worst_leaf_beats(double ma, long long ia, double mb, long long ib) {
    return ma < mb || (ma == mb && ia < ib);
}

}  // namespace

extern "C" {

const char* ehm_invariance_last_error(void) { return v_err.c_str(); }

int ehm_invariance_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_invariance_opts),
                           (int64_t)sizeof(ehm_invariance_result),
                           (int64_t)sizeof(ehm_invariance_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_compiled_successors(ehm_compiled* law, const ehm_invariance_opts* o,
                            ehm_invariance_result* res, const ehm_invariance_leaves* lv) {
    if (!law || !o || !res || !lv) return v_err.fail(EHM_E_INVALID, "successors: bad argument");
    if (o->n < 0 || o->chunk < 0) return v_err.fail(EHM_E_INVALID, "successors: n or chunk < 0");
    if (!o->root_vertices || !o->A || !o->B || !o->w || !o->leaf_mode)
        return v_err.fail(EHM_E_INVALID, "successors: a required array is NULL");
    if (o->n > 0 && (!lv->status || !lv->margin || !lv->worst || !lv->max_violation))
        return v_err.fail(EHM_E_INVALID, "successors: a required output is NULL");
    if (!(o->tol_exit >= 0.0))
        return v_err.fail(EHM_E_INVALID, "successors: tol_exit must be >= 0");
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law_shape(v_err, v, "successors");
    if (rc) return rc;
    const int p = v.p, n_u = v.n_u;
    rc = check_step_plant(v_err, o, n_u, EHM_R_MAX_D, "successors");
    if (rc) return rc;
    if (o->n_g < 0 || o->n_g > EHM_R_MAX_ROWS || (o->n_g > 0 && (!o->Gx || !o->gx)))
        return v_err.fail(EHM_E_INVALID, "successors: n_g = %d (0..%d)", (int)o->n_g,
                          EHM_R_MAX_ROWS);
    DevPlant pl{};
    int rows = 0;
    for (int m = 0; m < o->n_modes; ++m) {
        const int r = o->region_rows ? o->region_rows[m] : 0;
        if (r < 0) return v_err.fail(EHM_E_INVALID, "successors: mode %d has %d region rows", m, r);
        pl.row0[m] = rows;
        rows += r;
    }
    if (rows > EHM_R_MAX_ROWS || (rows > 0 && (!o->H || !o->h)))
        return v_err.fail(EHM_E_INVALID, "successors: %d mode-region rows (0..%d)", rows,
                          EHM_R_MAX_ROWS);
    for (int m = o->n_modes; m <= EHM_R_MAX_MODES; ++m) pl.row0[m] = rows;
    rc = check_law_leaves(v_err, v, o->n, o->leaf_ids, "successors");
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->worst_leaf = -1;
    res->worst_margin = NAN;
    if (o->n == 0) return EHM_OK;
    // the plant's doubles and the box, the region rows and the state rows after them
    const int n_c = 1 << o->n_d;
    Pack pk;
    int o_lo, o_hi;
    pack_step_plant(pk, pl, o, p, n_u, o_lo, o_hi);
    pl.n_g = o->n_g;
    pl.oH = pk.put(o->H, (size_t)rows * p);
    pl.oh = pk.put(o->h, (size_t)rows);
    pl.oG = pk.put(o->Gx, (size_t)o->n_g * p);
    pl.og = pk.put(o->gx, (size_t)o->n_g);
    pl.total = (int)pk.buf.size();
    const size_t plant_bytes = (size_t)pl.total * sizeof(double);
    const size_t lds = plant_bytes + EHM_INV_STATUSES * sizeof(unsigned int);
    EHM_HIP_TRY(v_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(v_err, stream.create());
    const size_t cell = (size_t)(p + 1) * p, pts = (size_t)(p + 1) * n_c;
    ParentTable T;
    EHM_HIP_TRY(v_err, make_parents(v, stream, T));
    const long long chunk =
        o->chunk > 0 ? o->chunk
                     : std::max<long long>(EHM_INV_BLOCK, std::min<long long>(
                                               65536, EHM_INV_BUDGET / (long long)(pts * p)));
    const size_t cap = (size_t)std::min<long long>(chunk, o->n);
    DevBuf d_plant, d_mode, d_roots, d_ids, d_cnt;
    EHM_HIP_TRY(v_err, d_plant.upload(pk.buf.data(), plant_bytes));
    pl.data = d_plant.as<const double>();
    EHM_HIP_TRY(v_err, d_mode.upload(o->leaf_mode, (size_t)v.n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(v_err, d_roots.upload(o->root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    if (o->leaf_ids) EHM_HIP_TRY(v_err, d_ids.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(v_err, d_cnt.alloc(EHM_INV_STATUSES * sizeof(unsigned long long)));
    EHM_HIP_TRY(v_err, hipMemsetAsync(d_cnt.ptr, 0, EHM_INV_STATUSES * sizeof(unsigned long long),
                                      stream));
    // a pass sets n and first; the outputs follow
    SuccArgs A{0, d_ids.as<const int32_t>(), 0, v.node, v.leaf_rec, v.root_entry, v.root_rec, v.nbr,
               d_roots.as<const double>(), T.view(), d_mode.as<const int32_t>(), n_u,
               v.leaf_stride, v.side_stride, (int)v.n_roots, o->n_d, o_lo, o_hi, o->tol_exit};
    A.counters = d_cnt.as<unsigned long long>();
    std::vector<double> hvert(cap * cell), vsub;
    // the per-leaf outputs: host array (nullptr: not asked for), the SuccArgs pointer its device
    // buffer goes to, bytes per leaf; the cells alone come a chunk at a time, for the volumes
    const size_t D = sizeof(double), I = sizeof(int32_t);
    struct Out {
        void* host;
        void* field;
        size_t bytes;
        bool per_chunk;
        DevBuf buf;
    } out[] = {
        {hvert.data(), &A.vertices, cell * D, true},
        {lv->status, &A.status, I},
        {lv->margin, &A.margin, D},
        {lv->worst, &A.worst, I},
        {lv->max_violation, &A.max_violation, D},
        {lv->x_next, &A.x_next, pts * p * D},
        {lv->succ_root, &A.succ_root, pts * I},
        {lv->succ_leaf, &A.succ_leaf, pts * I},
    };
    for (Out& t : out)
        if (t.host) {
            EHM_HIP_TRY(v_err, t.buf.alloc(cap * t.bytes));
            std::memcpy(t.field, &t.buf.ptr, sizeof t.buf.ptr);
        }
    std::vector<long long> has;
    EventPair ev;
    bool have_worst = false;
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        if (o->leaf_ids)
            EHM_HIP_TRY(v_err, hipMemcpyAsync(d_ids.ptr, o->leaf_ids + off,
                                              (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice,
                                              stream));
        A.n = nc;
        A.first = off;
        const dim3 grid(blocks_of(nc, EHM_INV_BLOCK)), block(EHM_INV_BLOCK);
        (void)hipEventRecord(ev.e0, stream);
        hipLaunchKernelGGL((v.single ? k_succ32 : k_succ64)[p - 1], grid, block, lds, stream, A,
                           pl);
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(v_err, hipGetLastError());
        for (const Out& t : out)
            if (t.host)
                EHM_HIP_TRY(v_err, hipMemcpyAsync(static_cast<char*>(t.host) +
                                                      (t.per_chunk ? 0 : (size_t)off * t.bytes),
                                                  t.buf.ptr, (size_t)nc * t.bytes,
                                                  hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(v_err, hipStreamSynchronize(stream));
        double s = 0.0;
        ev.seconds(&s);
        res->seconds += s;
        // the worst leaf and the volumes, in leaf order
        has.clear();
        for (long long q = 0; q < nc; ++q) {
            const int st = lv->status[off + q];
            const double mg = lv->margin[off + q];
            if ((st == INV_INVARIANT || st == INV_EXITS) && mg == mg &&
                (!have_worst || worst_leaf_beats(mg, off + q, res->worst_margin,
                                                 res->worst_leaf))) {
                have_worst = true;
                res->worst_margin = mg;
                res->worst_leaf = off + q;
            }
            if (st != INV_NO_CELL) has.push_back(q);
        }
        rc = cell_volumes(v_err, "successors", v.device, p, hvert.data(), has, vsub);
        if (rc) return rc;
        for (size_t a = 0; a < has.size(); ++a) {
            res->cell_volume += vsub[a];
            if (lv->status[off + has[a]] == INV_INVARIANT) res->invariant_volume += vsub[a];
        }
    }
    unsigned long long cnt[EHM_INV_STATUSES];
    EHM_HIP_TRY(v_err, hipMemcpy(cnt, d_cnt.ptr, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < EHM_INV_STATUSES; ++i) res->counts[i] = (int64_t)cnt[i];
    return EHM_OK;
}

}  // extern "C"
