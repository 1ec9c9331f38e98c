// ndp_kpconv.inc -- the input builder of KPConv-style networks on stacked clouds (points [N][3], lengths [B]): voxel-grid barycentre
// subsampling (k_voxel_keys, sort, k_voxel_reduce) and a batched fixed-radius search whose rows are sorted by distance and cut to K
// (k_radius_grid, sort, k_radius_search); ndp_voxel_subsample / ndp_radius_search and their workspace queries.  DESIGN.md "KPConv
// inputs".  No floating-point atomics, every output element has one writer, every sum one fixed order: the same bits run to run.
//
// THE GRID IS A SORTED KEY TABLE.  A point's cell is packed into 64 bits, (cloud : 16 | iz : 16 | iy : 16 | ix : 16), the points are
// sorted by that key (rocPRIM's device radix sort: stable, so equal keys stay in ascending input index), and the unique keys with the
// start offset of each run (ukey, ustart) are the grid; a cell is found by binary search.  Memory is O(N) whatever the bounding box:
// one far outlier costs one table entry.  The cloud is the key's top field, so a cloud never sees another cloud's cells.  What does
// not fit 16 bits per axis (or B > 65535) is refused, never wrapped: k_kp_bounds tests every cloud's extent before a key is formed.
//
// VOXEL MEMBERSHIP is the reference's (grid_subsampling.cpp:27, :53-55), all in fp32 and under -ffp-contract=off:
//   origin = floorf(min * (1 / dl)) * dl per cloud and axis,   i = floorf((p - origin) / dl).
// fp32 division is correctly rounded, so these are the host's bits.  origin can round to just above min, and i is then -1: the key
// stores i + 1, and -1 is a voxel like any other.  A barycentre is the sum of the voxel's points in ascending input index, in double,
// divided by the count and rounded to fp32 once (the reference sums in fp32).  Output order: per cloud ascending (iz, iy, ix), i.e.
// ascending key; max_p > 0 keeps the first max_p voxels of that order per cloud, and `inverse` is -1 for a point of a dropped voxel.
//
// RADIUS SEARCH.  Supports are binned per cloud into cells of edge  cell = radius * KP_CELL_MARGIN  (fp32), cell index
// c(p) = floorf((p - o) / cell) with o the cloud's support minimum; a query walks the 3 x 3 x 3 cells around its own, the three
// x-neighbours of a (z, y) pair as ONE key range (they are adjacent in key order).  Queries are processed in the order of their own
// cell keys, so the lanes of a wave walk the same cells.  A distance is k_knn's chain: d = q - s per axis,
// fmaf(dz, dz, fmaf(dy, dy, dx * dx)); a support is a neighbour iff d2 < r2 = radius * radius (strict, as nanoflann).  A lane keeps the
// KC in {16, 32, 64} >= K nearest in registers, ordered by (d2, index) whatever order the cells deliver them in.
//
// WHY NO NEIGHBOUR IS MISSED.  Cell indices are computed in fp32, so two points less than `radius` apart could land two computed cells
// apart if the cell edge were the radius itself.  Take a query q and a support s of its cloud with computed d2 < r2.  On every axis
// |q - s| < radius * (1 + 2^-22): the subtraction, the three roundings of the chain and the rounding of r2 are at most 6 relative
// errors of 2^-24 on the square, the square root halves them.  Let u(p) = (p - o) / cell in exact arithmetic.  The computed value
// u^(p) = fl(fl(p - o) / cell) is two correctly rounded operations, so |u^(p) - u(p)| <= |u(p)| * 2^-22.9.  Every support has
// 0 <= u^ < 65536 (k_kp_bounds refuses the call otherwise), and a query with a neighbour lies within 1 of it in u, so for both the
// error is below 0.009 cells.  Hence  |u^(q) - u^(s)| < (1 + 2^-22) * (1 + 2^-23) / KP_CELL_MARGIN + 0.018 = 0.9697.. + 0.018 < 1
// for KP_CELL_MARGIN = 1 + 1/32 (the middle factor is the rounding of `cell` itself).  Two numbers less than 1 apart have floors at
// most 1 apart: s lies in one of the 27 cells walked.  The margin costs (1 + 1/32)^3 = 1.097 x the candidates of an exact-radius cell.
//   Queries need not lie in the supports' box.  Their u^ is held to [-2, 65536] before it becomes an integer, which only adds cells
// to a walk that would otherwise meet none (below -2 every walked cell is negative, above 65536 every one is past the last a support
// can have): a far query gets an empty row, not a wrapped key.  NaN and infinite coordinates are refused.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <vector>

#define KP_MAX_CELL 65535              // largest stored cell field (16 bits per axis)
#define KP_MAX_K 64
#define KP_MAX_POINTS (1 << 30)
#define KP_MAX_F 4096
#define KP_CELL_MARGIN 1.03125f
#define KP_ST_NONFINITE 1              // status bits raised by the kernels, read back by the host entry
#define KP_ST_RANGE 2
#define KP_ST_QUERY_NONFINITE 4
typedef unsigned long long kp_u64;

__device__ __forceinline__ kp_u64 kp_key(int b, int iz, int iy, int ix) {
    return ((kp_u64)b << 48) | ((kp_u64)iz << 32) | ((kp_u64)iy << 16) | (kp_u64)ix;
}
// the cloud of stacked index i: the largest b with off[b] <= i (off [B + 1], off[0] = 0, strictly increasing)
__device__ __forceinline__ int kp_cloud_of(const int *off, int B, int i) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// stored cell field of one coordinate: floorf((p - o) / edge) + bias, held to 0..KP_MAX_CELL (k_kp_bounds has refused what would leave it)
__device__ __forceinline__ int kp_cell(float p, float o, float edge, int bias) {
    const float c = floorf((p - o) / edge) + (float)bias;
    return (int)fminf(fmaxf(c, 0.f), (float)KP_MAX_CELL);
}
__device__ __forceinline__ int kp_lower_bound(const kp_u64 *a, int n, kp_u64 key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per cloud: the cloud's minimum and maximum per axis, the grid origin geom[b] = {ox, oy, oz, 0} (voxel != 0: the
// reference's floorf(min * (1 / edge)) * edge; else the minimum itself) and the refusals: a coordinate that is not finite, or a
// cell field (index + bias) outside 0..KP_MAX_CELL.  The index is monotone in the coordinate, so the two ends bound every point.
extern "C" __global__ void __launch_bounds__(256)
k_kp_bounds(const float *pts, const int *off, float edge, int voxel, int bias, float *geom, int *status) {
    __shared__ float red[6][256];
    const int b = blockIdx.x, t = threadIdx.x, p0 = off[b], p1 = off[b + 1];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int i = p0 + t; i < p1; i += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * (size_t)i + a];
            bad |= !(fabsf(v) < INFINITY);
            mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v);
        }
    }
    if (bad) atomicOr(status, KP_ST_NONFINITE);
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[a][t] = mn[a]; red[3 + a][t] = mx[a]; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[a][t] = fminf(red[a][t], red[a][t + w]);
                red[3 + a][t] = fmaxf(red[3 + a][t], red[3 + a][t + w]);
            }
        }
        __syncthreads();
    }
    if (t < 3) {
        const float lo = red[t][0], hi = red[3 + t][0];
        const float o = voxel ? floorf(lo * (1.f / edge)) * edge : lo;
        geom[4 * b + t] = o;
        const float clo = floorf((lo - o) / edge) + (float)bias, chi = floorf((hi - o) / edge) + (float)bias;
        if (!(clo >= 0.f) || !(chi <= (float)KP_MAX_CELL)) atomicOr(status, KP_ST_RANGE);        // (written so that a NaN refuses)
    }
    if (t == 3) geom[4 * b + 3] = 0.f;
}

// key and payload of every point for the sort: key = (cloud, cell of the point in its cloud's grid), payload = its stacked index.
__device__ __forceinline__ void kp_point_key(const float *pts, const int *off, int B, const float *geom, float edge, int bias, int i,
                                             kp_u64 *keys, int *vals, int *status, int nonfinite_bit) {
    const int b = kp_cloud_of(off, B, i);
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (nonfinite_bit && !(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) atomicOr(status, nonfinite_bit);
    const float *o = geom + 4 * b;
    keys[i] = kp_key(b, kp_cell(z, o[2], edge, bias), kp_cell(y, o[1], edge, bias), kp_cell(x, o[0], edge, bias));
    vals[i] = i;
}
extern "C" __global__ void __launch_bounds__(256)
k_voxel_keys(const float *pts, int n, const int *off, int B, const float *geom, float dl, kp_u64 *keys, int *vals, int *status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) kp_point_key(pts, off, B, geom, dl, 1, i, keys, vals, status, 0);
}
// The same for the radius search's grid: supports (query == 0) and queries (query != 0: against the SUPPORTS' origins of their cloud,
// cells held to the key's range -- this key only orders the queries -- and their coordinates tested for NaN / infinity here).
extern "C" __global__ void __launch_bounds__(256)
k_radius_grid(const float *pts, int n, const int *off, int B, const float *geom, float cell, int query, kp_u64 *keys, int *vals, int *status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) kp_point_key(pts, off, B, geom, cell, 0, i, keys, vals, status, query ? KP_ST_QUERY_NONFINITE : 0);
}

// head[p] = 1 where a new key starts in the sorted keys; its inclusive scan is the 1-based number of the run p belongs to.
extern "C" __global__ void __launch_bounds__(256)
k_kp_heads(const kp_u64 *keys, int n, int *head) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) head[p] = p == 0 || keys[p] != keys[p - 1];
}
// the table: ustart[v] = first sorted position of run v, ustart[nU] = n, ukey[v] its key (may be NULL), meta[0] = nU.
extern "C" __global__ void __launch_bounds__(256)
k_kp_table(const kp_u64 *keys, const int *rank1, int n, kp_u64 *ukey, int *ustart, int *meta) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (p == 0 || keys[p] != keys[p - 1]) {
        const int v = rank1[p] - 1;
        ustart[v] = p;
        if (ukey) ukey[v] = keys[p];
    }
    if (p == n - 1) { ustart[rank1[p]] = n; meta[0] = rank1[p]; }
}

// per cloud: its first voxel and the offsets of its kept voxels in the output (one thread: B is small and the loads are independent)
extern "C" __global__ void k_voxel_layout(const int *rank1, const int *off, int B, int max_p, const int *meta, int *vfirst, int *out_off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int acc = 0;
    out_off[0] = 0;
    for (int b = 0; b < B; ++b) {
        const int first = rank1[off[b]] - 1;
        const int next = b + 1 < B ? rank1[off[b + 1]] - 1 : meta[0];
        const int count = next - first;
        vfirst[b] = first;
        acc += max_p > 0 && count > max_p ? max_p : count;
        out_off[b + 1] = acc;
    }
}

// One thread per (voxel, channel): channel 0..2 the coordinates, 3.. the features.  The run of the voxel is summed in sorted order,
// which within a run is ascending input index (stable sort), in double; one division, one rounding.
extern "C" __global__ void __launch_bounds__(256)
k_voxel_reduce(const float *pts, const float *feat, int F, const kp_u64 *keys, const int *idx, const int *ustart, const int *meta,
               const int *vfirst, const int *out_off, float *out_pts, float *out_feat) {
    const int C = 3 + F;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long v = g / C;
    const int c = (int)(g - v * C);
    if (v >= meta[0]) return;
    const int p0 = ustart[v], p1 = ustart[v + 1];
    const int b = (int)(keys[p0] >> 48);
    const int vl = (int)v - vfirst[b];
    if (vl >= out_off[b + 1] - out_off[b]) return;                      // beyond max_p
    const size_t o = (size_t)(out_off[b] + vl);
    double acc = 0.0;
    if (c < 3) {
        for (int p = p0; p < p1; ++p) acc += (double)pts[3 * (size_t)idx[p] + c];
        out_pts[3 * o + c] = (float)(acc / (double)(p1 - p0));
    } else {
        for (int p = p0; p < p1; ++p) acc += (double)feat[(size_t)idx[p] * F + (c - 3)];
        out_feat[o * F + (c - 3)] = (float)(acc / (double)(p1 - p0));
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_voxel_inverse(const kp_u64 *keys, const int *idx, const int *rank1, int n, const int *vfirst, const int *out_off, int *inverse) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int b = (int)(keys[p] >> 48);
    const int vl = rank1[p] - 1 - vfirst[b];
    inverse[idx[p]] = vl < out_off[b + 1] - out_off[b] ? out_off[b] + vl : -1;
}

// the supports in cell order as {x, y, z, index bits}: one 16-byte load per candidate in the search
extern "C" __global__ void __launch_bounds__(256)
k_radius_records(const float *s, const int *idx, int n, float4 *rec) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = idx[p];
    rec[p] = make_float4(s[3 * (size_t)i], s[3 * (size_t)i + 1], s[3 * (size_t)i + 2], __int_as_float(i));
}

// (d, j) enters the list ordered by (d2, index); entries past KC fall off.  Empty slots are (inf, INT_MAX): every candidate precedes them.
template <int KC>
__device__ __forceinline__ void kp_insert(float (&ld)[KC], int (&li)[KC], float d, int j) {
#pragma unroll
    for (int k = KC - 1; k > 0; --k) {                                   // top down: entries k - 1 and k are still the old ones
        const bool up = ld[k - 1] > d || (ld[k - 1] == d && li[k - 1] > j);
        const bool here = ld[k] > d || (ld[k] == d && li[k] > j);
        li[k] = up ? li[k - 1] : here ? j : li[k];
        ld[k] = up ? ld[k - 1] : here ? d : ld[k];
    }
    if (ld[0] > d || (ld[0] == d && li[0] > j)) { ld[0] = d; li[0] = j; }
}

// One query per lane, in the order of the queries' cell keys.  KC = 0: counts only.
template <int KC>
__global__ void __launch_bounds__(64)
k_radius_search(const float *q, int nq, const int *order, const int *qoff, int B, const float *geom, float cell, float r2,
                const kp_u64 *ukey, const int *ustart, const int *meta, const float4 *rec, int K, int shadow,
                int *idx_out, float *d2_out, int *counts) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= nq) return;
    const int qi = order[t];
    const int b = kp_cloud_of(qoff, B, qi);
    const float qx = q[3 * (size_t)qi], qy = q[3 * (size_t)qi + 1], qz = q[3 * (size_t)qi + 2];
    const float *o = geom + 4 * b;
    const int cx = (int)fminf(fmaxf(floorf((qx - o[0]) / cell), -2.f), 65536.f);
    const int cy = (int)fminf(fmaxf(floorf((qy - o[1]) / cell), -2.f), 65536.f);
    const int cz = (int)fminf(fmaxf(floorf((qz - o[2]) / cell), -2.f), 65536.f);
    const int nU = meta[0];
    constexpr int KA = KC > 0 ? KC : 1;
    float ld[KA];
    int li[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) { ld[k] = INFINITY; li[k] = 0x7fffffff; }
    int cnt = 0;
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, KP_MAX_CELL);
    if (x0 <= x1) {
        for (int z = max(cz - 1, 0); z <= min(cz + 1, KP_MAX_CELL); ++z) {
            for (int y = max(cy - 1, 0); y <= min(cy + 1, KP_MAX_CELL); ++y) {
                const int u0 = kp_lower_bound(ukey, nU, kp_key(b, z, y, x0));
                const int u1 = kp_lower_bound(ukey, nU, kp_key(b, z, y, x1) + 1);
                const int p1 = ustart[u1];
                for (int p = ustart[u0]; p < p1; ++p) {
                    const float4 r = rec[p];
                    const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
                    const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if (d < r2) {
                        ++cnt;
                        if constexpr (KC > 0) kp_insert<KA>(ld, li, d, __float_as_int(r.w));
                    }
                }
            }
        }
    }
    counts[qi] = cnt;
    if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (k < K) {
                const bool have = k < cnt;
                idx_out[(size_t)qi * K + k] = have ? li[k] : shadow;
                if (d2_out) d2_out[(size_t)qi * K + k] = have ? ld[k] : INFINITY;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host entries
// ------------------------------------------------------------------------------------------------
// rocPRIM names its temporary size only with a device present, and the workspace queries must answer without one.  So they use a
// bound read off its layout (device_radix_sort.hpp: key and value double buffers 12 n, look-back states < 8 n + 2 KiB, digit tables
// < 32 KiB; the scan's look-back states are far smaller), and the entries compare rocPRIM's own figure with it and refuse if it is ever larger.
static long long kp_sort_temp_bound(long long n) { return 24 * n + (256 << 10); }

struct KpCarve {                       // 16-byte aligned pieces of a workspace, the same walk for the size query and the entry
    char *base;
    long long at = 0;
    explicit KpCarve(void *ws) : base((char *)ws) {}
    template <class T> T *take(long long count) {
        T *p = (T *)(base + at);
        at += (count * (long long)sizeof(T) + 15) / 16 * 16;
        return p;
    }
};

// lengths [B] on the host -> offsets [B + 1] and their total, which may not exceed n_max
static int kp_check_lengths(const char *who, const int *len, int B, long long n_max, long long *n_out, std::vector<int> *off) {
    if (int rc = check_batch(who, len, B)) return rc;
    long long n = 0;
    off->assign(1, 0);
    for (int b = 0; b < B; ++b) {
        if (len[b] < 1) return failf(NDP_E_INVALID, "%s: every length must be >= 1 (cloud %d has %d)", who, b, len[b]);
        n += len[b];
        if (n > n_max) return failf(NDP_E_UNSUPPORTED, "%s: at most %lld points in all", who, n_max);
        off->push_back((int)n);
    }
    *n_out = n;
    return 0;
}

static int kp_sort(void *tmp, long long tmp_bytes, kp_u64 *ki, kp_u64 *ko, int *vi, int *vo, int n, int B, hipStream_t s) {
    int end_bit = 48;
    while (end_bit < 64 && (1LL << (end_bit - 48)) < B) ++end_bit;
    size_t need = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, ki, ko, vi, vo, (unsigned)n, 0u, (unsigned)end_bit, s), "radix sort (size query)");
    if ((long long)need > tmp_bytes) return fail(NDP_E_UNSUPPORTED, "the key sort asks for more temporary storage than the workspace bound allows");
    HIP_TRY(rocprim::radix_sort_pairs(tmp, need, ki, ko, vi, vo, (unsigned)n, 0u, (unsigned)end_bit, s), "radix sort");
    return 0;
}

// sorted keys -> rank1 (1-based run number per position), ustart / ukey / meta[0] = nU
static int kp_table(void *tmp, long long tmp_bytes, const kp_u64 *keys, int n, int *rank1, kp_u64 *ukey, int *ustart, int *meta, hipStream_t s) {
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(k_kp_heads, grid, block, 0, s, keys, n, rank1);
    HIP_TRY(hipGetLastError(), "k_kp_heads launch");
    size_t need = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, need, rank1, rank1, (size_t)n, rocprim::plus<int>(), s), "scan (size query)");
    if ((long long)need > tmp_bytes) return fail(NDP_E_UNSUPPORTED, "the scan asks for more temporary storage than the workspace bound allows");
    HIP_TRY(rocprim::inclusive_scan(tmp, need, rank1, rank1, (size_t)n, rocprim::plus<int>(), s), "scan");
    hipLaunchKernelGGL(k_kp_table, grid, block, 0, s, keys, (const int *)rank1, n, ukey, ustart, meta);
    HIP_TRY(hipGetLastError(), "k_kp_table launch");
    return 0;
}

static int kp_status_fail(const char *who, int st, const char *what_range) {
    static thread_local char msg[200];
    if (st & KP_ST_NONFINITE) snprintf(msg, sizeof msg, "%s: a coordinate is NaN or infinite", who);
    else if (st & KP_ST_QUERY_NONFINITE) snprintf(msg, sizeof msg, "%s: a query coordinate is NaN or infinite", who);
    else snprintf(msg, sizeof msg, "%s: a cloud spans more than %d %s along an axis (the 64-bit cell key holds 16 bits per axis)", who, KP_MAX_CELL, what_range);
    return fail(st & KP_ST_RANGE && !(st & (KP_ST_NONFINITE | KP_ST_QUERY_NONFINITE)) ? NDP_E_UNSUPPORTED : NDP_E_INVALID, msg);
}

struct KpVoxelWs {
    int *status, *off, *vfirst, *out_off, *vals_a, *vals_b, *rank1, *ustart;
    float *geom;
    kp_u64 *keys_a, *keys_b;
    char *tmp;
    long long tmp_bytes, total;
    KpVoxelWs(void *ws, long long n, int B) {
        KpCarve c(ws);
        status = c.take<int>(16); off = c.take<int>(B + 1); vfirst = c.take<int>(B); out_off = c.take<int>(B + 1);
        geom = c.take<float>(4LL * B);
        keys_a = c.take<kp_u64>(n); keys_b = c.take<kp_u64>(n);
        vals_a = c.take<int>(n); vals_b = c.take<int>(n); rank1 = c.take<int>(n); ustart = c.take<int>(n + 1);
        tmp_bytes = kp_sort_temp_bound(n);
        tmp = c.take<char>(tmp_bytes);
        total = c.at;
    }
};

extern "C" int ndp_voxel_subsample_workspace(long long n, int B, long long *nbytes) {
    if (n < 1 || n > KP_MAX_POINTS || B < 1 || B > NDP_MAX_B || B > n || !nbytes)
        return fail(NDP_E_INVALID, "ndp_voxel_subsample_workspace: 1 <= B <= 65535, B <= n <= 2^30, nbytes not NULL");
    *nbytes = KpVoxelWs(nullptr, n, B).total;
    return 0;
}

extern "C" int ndp_voxel_subsample(const float *pts, const float *feat, int F, const int *lengths_host, int B, float dl, int max_p, void *ws,
                                   long long ws_bytes, float *out_pts, float *out_feat, int *inverse, int *out_lengths_host, void *stream) {
    std::vector<int> off;
    long long n = 0;
    if (int rc = kp_check_lengths("ndp_voxel_subsample", lengths_host, B, KP_MAX_POINTS, &n, &off)) return rc;
    if (!(dl > 0.f) || !std::isfinite(dl)) return fail(NDP_E_INVALID, "ndp_voxel_subsample: dl must be positive and finite");
    if (F < 0 || F > KP_MAX_F) return fail(NDP_E_INVALID, "ndp_voxel_subsample: F must lie in 0..4096");
    if (n * (3 + F) > (1LL << 38)) return fail(NDP_E_UNSUPPORTED, "ndp_voxel_subsample: n * (3 + F) must not exceed 2^38");
    if (!pts || !ws || !out_pts || !out_lengths_host || (F > 0 && (!feat || !out_feat)))
        return fail(NDP_E_INVALID, "ndp_voxel_subsample: null pointer");
    if (!aligned16(ws)) return fail(NDP_E_INVALID, "ndp_voxel_subsample: the workspace must be 16-byte aligned");
    KpVoxelWs w(ws, n, B);
    if (ws_bytes < w.total) return fail(NDP_E_INVALID, "ndp_voxel_subsample: workspace smaller than ndp_voxel_subsample_workspace(n, B)");
    hipStream_t s = (hipStream_t)stream;
    const int N = (int)n;
    const dim3 grid((N + 255) / 256), block(256);
    HIP_TRY(hipMemsetAsync(w.status, 0, 64, s), "hipMemsetAsync");
    HIP_TRY(hipMemcpyAsync(w.off, off.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, s), "hipMemcpyAsync (offsets)");
    hipLaunchKernelGGL(k_kp_bounds, dim3(B), block, 0, s, pts, (const int *)w.off, dl, 1, 1, w.geom, w.status);
    hipLaunchKernelGGL(k_voxel_keys, grid, block, 0, s, pts, N, (const int *)w.off, B, (const float *)w.geom, dl, w.keys_a, w.vals_a, w.status);
    HIP_TRY(hipGetLastError(), "k_voxel_keys launch");
    if (int rc = kp_sort(w.tmp, w.tmp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, N, B, s)) return rc;
    if (int rc = kp_table(w.tmp, w.tmp_bytes, w.keys_b, N, w.rank1, nullptr, w.ustart, w.status + 4, s)) return rc;
    hipLaunchKernelGGL(k_voxel_layout, dim3(1), dim3(64), 0, s, (const int *)w.rank1, (const int *)w.off, B, max_p, (const int *)(w.status + 4), w.vfirst, w.out_off);
    const long long work = n * (3 + F);
    hipLaunchKernelGGL(k_voxel_reduce, dim3((unsigned)((work + 255) / 256)), block, 0, s, pts, feat, F, (const kp_u64 *)w.keys_b, (const int *)w.vals_b,
                       (const int *)w.ustart, (const int *)(w.status + 4), (const int *)w.vfirst, (const int *)w.out_off, out_pts, out_feat);
    if (inverse)
        hipLaunchKernelGGL(k_voxel_inverse, grid, block, 0, s, (const kp_u64 *)w.keys_b, (const int *)w.vals_b, (const int *)w.rank1, N,
                           (const int *)w.vfirst, (const int *)w.out_off, inverse);
    HIP_TRY(hipGetLastError(), "k_voxel_reduce launch");
    std::vector<int> back(B + 2);                                        // the output's size is data: this entry ends in a synchronise
    HIP_TRY(hipMemcpyAsync(back.data(), w.out_off, sizeof(int) * (B + 1), hipMemcpyDeviceToHost, s), "hipMemcpyAsync (lengths)");
    HIP_TRY(hipMemcpyAsync(back.data() + B + 1, w.status, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync (status)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (back[B + 1]) return kp_status_fail("ndp_voxel_subsample", back[B + 1], "voxels");
    for (int b = 0; b < B; ++b) out_lengths_host[b] = back[b + 1] - back[b];
    return 0;
}

struct KpRadiusWs {
    int *status, *qoff, *soff, *vals_a, *vals_b, *rank1, *ustart;
    float *geom;
    float4 *rec;
    kp_u64 *keys_a, *keys_b, *ukey;
    char *tmp;
    long long tmp_bytes, total;
    KpRadiusWs(void *ws, long long nq, long long ns, int B) {
        const long long m = std::max(nq, ns);
        KpCarve c(ws);
        status = c.take<int>(16); qoff = c.take<int>(B + 1); soff = c.take<int>(B + 1);
        geom = c.take<float>(4LL * B);
        rec = c.take<float4>(ns);
        keys_a = c.take<kp_u64>(m); keys_b = c.take<kp_u64>(m); ukey = c.take<kp_u64>(ns);
        vals_a = c.take<int>(m); vals_b = c.take<int>(m); rank1 = c.take<int>(ns); ustart = c.take<int>(ns + 1);
        tmp_bytes = kp_sort_temp_bound(m);
        tmp = c.take<char>(tmp_bytes);
        total = c.at;
    }
};

extern "C" int ndp_radius_search_workspace(long long nq, long long ns, int B, long long *nbytes) {
    if (nq < 1 || ns < 1 || nq > KP_MAX_POINTS || ns > KP_MAX_POINTS || B < 1 || B > NDP_MAX_B || B > nq || B > ns || !nbytes)
        return fail(NDP_E_INVALID, "ndp_radius_search_workspace: 1 <= B <= 65535, B <= nq, ns <= 2^30, nbytes not NULL");
    *nbytes = KpRadiusWs(nullptr, nq, ns, B).total;
    return 0;
}

extern "C" int ndp_radius_search(const float *q, const float *sup, const int *q_lengths_host, const int *s_lengths_host, int B, float radius,
                                 int K, void *ws, long long ws_bytes, int *idx, float *d2, int *counts, void *stream) {
    std::vector<int> qoff, soff;
    long long nq = 0, ns = 0;
    if (int rc = kp_check_lengths("ndp_radius_search (queries)", q_lengths_host, B, KP_MAX_POINTS, &nq, &qoff)) return rc;
    if (int rc = kp_check_lengths("ndp_radius_search (supports)", s_lengths_host, B, KP_MAX_POINTS, &ns, &soff)) return rc;
    if (!(radius > 0.f) || !std::isfinite(radius)) return fail(NDP_E_INVALID, "ndp_radius_search: radius must be positive and finite");
    if (K < 0 || K > KP_MAX_K) return fail(NDP_E_INVALID, "ndp_radius_search: K must lie in 0..64 (0: counts only)");
    if (!q || !sup || !ws || !counts || (K > 0 && !idx)) return fail(NDP_E_INVALID, "ndp_radius_search: null pointer");
    if (!aligned16(ws)) return fail(NDP_E_INVALID, "ndp_radius_search: the workspace must be 16-byte aligned");
    const float cell = radius * KP_CELL_MARGIN, r2 = radius * radius;
    if (!std::isfinite(cell) || !(r2 > 0.f) || !std::isfinite(r2)) return fail(NDP_E_INVALID, "ndp_radius_search: radius * radius must be a positive finite fp32");
    KpRadiusWs w(ws, nq, ns, B);
    if (ws_bytes < w.total) return fail(NDP_E_INVALID, "ndp_radius_search: workspace smaller than ndp_radius_search_workspace(nq, ns, B)");
    hipStream_t s = (hipStream_t)stream;
    const int NQ = (int)nq, NS = (int)ns;
    const dim3 gq((NQ + 255) / 256), gs((NS + 255) / 256), block(256);
    int *meta = w.status + 4;
    HIP_TRY(hipMemsetAsync(w.status, 0, 64, s), "hipMemsetAsync");
    HIP_TRY(hipMemcpyAsync(w.qoff, qoff.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, s), "hipMemcpyAsync (offsets)");
    HIP_TRY(hipMemcpyAsync(w.soff, soff.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, s), "hipMemcpyAsync (offsets)");
    // the supports' grid
    hipLaunchKernelGGL(k_kp_bounds, dim3(B), block, 0, s, sup, (const int *)w.soff, cell, 0, 0, w.geom, w.status);
    hipLaunchKernelGGL(k_radius_grid, gs, block, 0, s, sup, NS, (const int *)w.soff, B, (const float *)w.geom, cell, 0, w.keys_a, w.vals_a, w.status);
    HIP_TRY(hipGetLastError(), "k_radius_grid launch");
    if (int rc = kp_sort(w.tmp, w.tmp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, NS, B, s)) return rc;
    if (int rc = kp_table(w.tmp, w.tmp_bytes, w.keys_b, NS, w.rank1, w.ukey, w.ustart, meta, s)) return rc;
    hipLaunchKernelGGL(k_radius_records, gs, block, 0, s, sup, (const int *)w.vals_b, NS, w.rec);
    // the queries in the order of their cells (keys_b / vals_b are free again: the stream orders the launches)
    hipLaunchKernelGGL(k_radius_grid, gq, block, 0, s, q, NQ, (const int *)w.qoff, B, (const float *)w.geom, cell, 1, w.keys_a, w.vals_a, w.status);
    HIP_TRY(hipGetLastError(), "k_radius_grid launch");
    if (int rc = kp_sort(w.tmp, w.tmp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, NQ, B, s)) return rc;
    const dim3 grid((NQ + 63) / 64), wave(64);
#define KP_SEARCH(KC)                                                                                                             \
    hipLaunchKernelGGL(k_radius_search<KC>, grid, wave, 0, s, q, NQ, (const int *)w.vals_b, (const int *)w.qoff, B, (const float *)w.geom, cell, r2, \
                       (const kp_u64 *)w.ukey, (const int *)w.ustart, (const int *)meta, (const float4 *)w.rec, K, NS, idx, d2, counts)
    if (K == 0) KP_SEARCH(0);
    else if (K <= 16) KP_SEARCH(16);
    else if (K <= 32) KP_SEARCH(32);
    else KP_SEARCH(64);
#undef KP_SEARCH
    HIP_TRY(hipGetLastError(), "k_radius_search launch");
    int st = 0;                                                          // the refusals are found on the device: this entry ends in a synchronise
    HIP_TRY(hipMemcpyAsync(&st, w.status, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync (status)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (st) return kp_status_fail("ndp_radius_search", st, "cells of one radius");
    return 0;
}
