// Rebuild / Decode of segments that each bring their own share set, in one
// stream-ordered pass (rs_sets.hpp).  Reference: the per-segment Rebuild of
// StripeReader (private/eestream/stripe.go:382-428), each download's own share
// set (stripe.go:314-354, private/ecclient/client.go:273-308).
//
//  rs_sets_prep: one workgroup per segment.  G is the Lagrange basis on the
//      points x_0 = 0, x_i = alpha^(i-1) (G[i][j] = L_j(x_i), gf256_field.hpp),
//      so the inverse of the k rows of the basis shares S -- what infectious
//      Rebuild inverts per stripe -- is interpolation through S's points: data
//      d = sum over s in S of share_s * L^S_s(x_d), and a share u (Decode's
//      syndrome rows) is predicted the same way at x_u.  In closed form,
//          L^S_s(y) = N(y) / ((y - x_s) W_s),  N(y) = prod_t (y - x_t),
//          W_s = prod_{t != s} (x_s - x_t),
//      i.e. sums of logarithms and one exp per coefficient: independent table
//      lookups, no elimination (a Gauss-Jordan in LDS measured ~60 us per
//      segment, the lookups a few).  The inverse is unique, so the bytes are
//      those of the k x k inversion (tests: against the oracle's, which
//      inverts).  Then the rows' jump-table leaf addresses, in the layout
//      rs_matmul_sets reads ([pass][input][group][8], rows right-aligned per
//      group).
//  rs_matmul_sets<NW>: the share-set tile body (rs_sets_tile.hpp share_tile)
//      with this call's geometry (SetsGeom): every segment the same size, the
//      tile's segment descriptor giving input pointers, copy-through and row
//      offsets and the leaf table; then the call's completion count.
#include <hip/hip_runtime.h>

#include "../../include/uplink_ec.h"
#include "gf256_field.hpp"
#include "rs_device.hpp"
#include "rs_kernels.hpp"
#include "rs_sets.hpp"
#include "rs_sets_tile.hpp"

namespace uplink_ec {
namespace {

using namespace dev;

__constant__ GfTables c_gf = make_gf_tables();

// One segment's decode rows, solved and written as leaf addresses by one
// workgroup (rs_sets_prep).
__device__ __forceinline__ void solve_rows(const SetStage *st, uint64_t jt_base) {
    __shared__ uint8_t s_exp[512], s_log[256];
    __shared__ uint8_t s_x[kMaxOps];                    // basis points x_p
    __shared__ uint8_t s_y[2 * kMaxOps];                // row points y_r
    __shared__ int16_t s_lw[kMaxOps];                   // log W_p
    __shared__ int16_t s_ln[2 * kMaxOps], s_hit[2 * kMaxOps];  // log N_r, or the basis position row r sits on
    __shared__ int s_num[kMaxOps], s_miss[kMaxOps];
    __shared__ int s_acc[kMaxOps + 2 * kMaxOps];  // the sums of logarithms of W_p, then of N_r
    __shared__ int s_hdr[8];
    __shared__ uint64_t *s_tgt;
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    for (int i = tid; i < kMaxOps; i += nt) {
        s_num[i] = st->num[i];
        s_miss[i] = st->missing[i];
    }
    if (tid == 0) s_hdr[0] = st->d.nin;
    if (tid == 1) s_hdr[1] = st->d.nout;
    if (tid == 2) s_hdr[2] = st->d.nstore;
    if (tid == 3) s_hdr[3] = st->nw;
    if (tid == 4) s_hdr[4] = st->k;
    if (tid == 5) s_tgt = st->d.tgt;
    for (int i = tid; i < 512; i += nt) s_exp[i] = c_gf.exp[i];
    for (int i = tid; i < 256; i += nt) s_log[i] = c_gf.log[i];
    __syncthreads();
    const int nin = s_hdr[0], nout = s_hdr[1], nstore = s_hdr[2], nw = s_hdr[3], k = s_hdr[4];
    auto point = [&](int num) -> uint8_t { return num == 0 ? 0 : s_exp[(num - 1) % 255]; };
    for (int i = tid; i < k; i += nt) s_x[i] = point(s_num[i]);
    // row r's point: a missing data position (its data index), or a non-basis share (a syndrome row)
    for (int i = tid; i < nout; i += nt) s_y[i] = point(i < nstore ? s_miss[i] : s_num[k + i - nstore]);
    // log W_p = sum over t != p of log(x_p ^ x_t) (the points are distinct: the host checked), and
    // log N_r = sum over t of log(y_r ^ x_t), a row whose point is a basis point being that share
    // itself: (k + nout) x k independent terms, spread over the workgroup and added in LDS
    // (one term per thread and step instead of a k-long chain per sum: 13 -> ~5 us per launch)
    for (int i = tid; i < k; i += nt) s_acc[i] = 0;
    for (int i = tid; i < nout; i += nt) {
        s_acc[kMaxOps + i] = 0;
        s_hit[i] = -1;
    }
    __syncthreads();
    for (int e = tid; e < (k + nout) * k; e += nt) {
        const int a = e / k, t = e - a * k;
        if (a < k) {
            if (t != a) atomicAdd(&s_acc[a], (int)s_log[s_x[a] ^ s_x[t]]);
        } else {
            const uint8_t d = s_y[a - k] ^ s_x[t];
            if (d) atomicAdd(&s_acc[kMaxOps + a - k], (int)s_log[d]);
            else s_hit[a - k] = (int16_t)t;
        }
    }
    __syncthreads();
    for (int i = tid; i < k; i += nt) s_lw[i] = (int16_t)(s_acc[i] % 255);
    for (int i = tid; i < nout; i += nt) s_ln[i] = (int16_t)(s_acc[kMaxOps + i] % 255);
    __syncthreads();
    // leaf addresses: coefficient of basis input j in row r is N_r / ((y_r ^ x_j) W_j) (Lagrange
    // interpolation through the basis points, evaluated at y_r); 1 on a non-basis input's own
    // syndrome row; else 0
    const int npass = npass_of(nout, nw), per_pass = nin * nw * kRows;
    uint64_t *tgt = s_tgt;
    for (int e = tid; e < npass * per_pass; e += nt) {
        const int pass = e / per_pass, rem = e - pass * per_pass;
        const int j = rem / (nw * kRows), g = (rem / kRows) % nw, o = rem % kRows;
        int rb, cn;
        rows_of(pass, npass, nout, nw, g, rb, cn);
        const int oo = o - (kRows - cn);
        uint32_t c = 0;
        if (oo >= 0) {
            const int r = rb + oo;
            if (j >= k) {
                c = (uint32_t)(r >= nstore && j - k == r - nstore);
            } else if (s_hit[r] >= 0) {
                c = (uint32_t)(s_hit[r] == j);
            } else {
                const int l = s_ln[r] - s_log[s_y[r] ^ s_x[j]] - s_lw[j];
                c = s_exp[((l % 255) + 255) % 255];
            }
        }
        tgt[e] = jt_base + (uint64_t)c * RS_JT_SLOT;
    }
}

__device__ __forceinline__ void prep_one(const SetStage *st, SetDesc *dd, uint64_t jt_base, uint32_t *done_ctr) {
    const int tid = threadIdx.x;
    copy_desc(&st->d, dd);
    if (tid == 6) {
        uint32_t *zc = st->d.zero_check;
        if (zc) *zc = 0u;
    }
    if (tid == 7 && blockIdx.x == 0 && done_ctr) *done_ctr = 0u;
    solve_rows(st, jt_base);
}

__global__ __launch_bounds__(256) void rs_sets_prep(const SetStage *stage, SetDesc *desc, uint64_t jt_base,
                                                    uint32_t *done_ctr) {
    prep_one(stage + blockIdx.x, desc + blockIdx.x, jt_base, done_ctr);
}

// One segment: its record passed as the kernel's argument (3.1 KB of the 4 KB a
// launch carries), so the prep reads nothing over the bus
__global__ __launch_bounds__(256) void rs_sets_prep1(const SetStage stage, SetDesc *desc, uint64_t jt_base,
                                                     uint32_t *done_ctr) {
    prep_one(&stage, desc, jt_base, done_ctr);
}

// The tile body's geometry (rs_sets_tile.hpp) of a call whose segments share
// one size, stripe-major out; D: ConstDesc (the segment's descriptor in device
// memory, its leaf table made by rs_sets_prep) or ConstOne (one segment,
// rs_sets_one: the record is the launch's arguments, and the workgroup writes
// the leaf table from the host's coefficients while its first chunk's loads
// are in flight -- every workgroup the same bytes -- and reads it back with
// scalar loads once its own stores are complete).  The descriptors are read
// through the constant address space: the kernel never writes them.
typedef const __attribute__((address_space(4))) SetDesc ConstDesc;
typedef const __attribute__((address_space(4))) SetOne ConstOne;

template <class D>
struct SetsGeom : StripeGeom<D> {
    static constexpr bool kOwnTable = __is_same(D, ConstOne);
    using StripeGeom<D>::d;
    const SetsArgs &a;

    __device__ __forceinline__ SetsGeom(const SetsArgs &a_, D *d_) : StripeGeom<D>{d_}, a(a_) {}
    __device__ __forceinline__ bool skip(int nin, int) const { return !(d->status == 0 && nin > 0); }
    // the tile's two chunks of 16 byte columns per lane (rs_tile.hpp tile_cols)
    __device__ __forceinline__ void cols(int lane) {
        const int64_t tile = blockIdx.x;
        const int64_t seg = kOwnTable ? 0 : tile / a.tiles_per_seg;
        this->stripe_cols((tile - seg * a.tiles_per_seg) * kTileChunks + lane, a.chunks_per_seg, a.cps, a.ess, a.k);
    }
    __device__ __forceinline__ bool in_ok(const uint8_t *p, const uint8_t *share) const {
        return in_span(a, p, share, a.nstripes * a.ess, 8);
    }
    __device__ __forceinline__ bool out_ok(const uint8_t *p, const uint8_t *) const {
        return in_span(a, p, this->out, a.nstripes * a.ess * a.k, 9);
    }
    // Every workgroup writes the whole table, the same bytes, and reads it only after its
    // own stores are complete: the chunk's vmcnt(0) waits for them with the loads, before
    // the barrier every wave passes ahead of its first scalar load of the table.
    // Whichever copy a read meets -- this XCD's L2 line, or the scalar cache's, filled by
    // a workgroup that had itself finished writing -- holds these bytes; the scalar cache
    // starts the launch empty, so nothing is left from the slot's previous call.
    template <int NW>
    __device__ __forceinline__ void write_table(int npass, int nin, int nout) const {
        uint64_t *t = d->tgt;
        for (int e = threadIdx.x; e < npass * nin * NW * kRows; e += NW * 64) {
            const int pass = e / (nin * NW * kRows), rem = e - pass * (nin * NW * kRows);
            const int j = rem / (NW * kRows), g = (rem / kRows) % NW, o = rem % kRows;
            int rb, cn;
            rows_of(pass, npass, nout, NW, g, rb, cn);
            const int oo = o - (kRows - cn);
            const uint32_t c = oo >= 0 ? d->coef[(rb + oo) * nin + j] : 0u;
            t[e] = a.jt_base + (uint64_t)c * RS_JT_SLOT;
        }
    }
};

// every wave of this workgroup has read all it reads from the slot (descriptor,
// leaf table) once it is past this barrier (no wait for the stores in flight)
__device__ __forceinline__ void sets_done(const SetsArgs &a) {
    if (a.done_ctr) {
        lds_barrier();
        if (threadIdx.x == 0) {
            const uint32_t old = atomicAdd(a.done_ctr, 1u);
            if (old + 1 == a.total_wgs) {
                atomicExch(a.done_ctr, 0u);
                __hip_atomic_store(a.host_done, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_matmul_sets(const SetsArgs a) {
    SetsGeom<ConstDesc> G{a, (ConstDesc *)(a.desc + blockIdx.x / a.tiles_per_seg)};
    share_tile<NW>(G);
    sets_done(a);
}

template <int NW>
__global__ __launch_bounds__(NW * 64, 4) void rs_sets_one(const SetOne p) {
    SetsGeom<ConstOne> G{p.a, (ConstOne *)&p};
    share_tile<NW>(G);
    sets_done(p.a);
}

}  // namespace

// as the straight-line split (rs_sl_codegen.cpp split_for): 15-16 rows on 3 waves, not 2 -- one
// share set of 15 rows, 32 segments: 794-848 against 821-866 us on 2 waves, 815-834 on 4
// (profiles/r05/r/); the 14-24-row mix of fresh sets on 4 waves instead of 3: 874-882 against
// 855-857 us, one segment 73.5 against 62-64 us wall (profiles/r05/q/)
int sets_waves(int rows) { return rows <= 14 ? 2 : rows <= 24 ? 3 : 4; }

hipError_t launch_sets_prep(const SetStage *stage, SetDesc *desc, int nseg, uint64_t jt_base, uint32_t *done_ctr,
                            hipStream_t s) {
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(rs_sets_prep, dim3(nseg), dim3(256), 0, s, stage, desc, jt_base, done_ctr);
    return hipGetLastError();
}

hipError_t launch_sets_prep1(const SetStage &stage, SetDesc *desc, uint64_t jt_base, uint32_t *done_ctr,
                             hipStream_t s) {
    hipLaunchKernelGGL(rs_sets_prep1, dim3(1), dim3(256), 0, s, stage, desc, jt_base, done_ctr);
    return hipGetLastError();
}

hipError_t launch_sets_one(const SetOne &p, int nw, hipStream_t s) {
    if (p.a.total_tiles <= 0) return hipSuccess;
    if (p.nin > kOneMaxIn || p.nin * p.nout > kOneMaxCoef) return hipErrorInvalidValue;
    return launch_share_tile(p, p.a.total_tiles, nw, s, rs_sets_one<2>, rs_sets_one<3>, rs_sets_one<4>);
}

hipError_t launch_matmul_sets(const SetsArgs &a, int nw, hipStream_t s) {
    return launch_share_tile(a, a.total_tiles, nw, s, rs_matmul_sets<2>, rs_matmul_sets<3>, rs_matmul_sets<4>);
}

}  // namespace uplink_ec
