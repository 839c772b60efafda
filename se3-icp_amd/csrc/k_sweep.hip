// k_sweep.hip — expansion of a shared setup into one group of a parameter sweep (gfx950).
//
// The shared setup (Engine::register_sweep) leaves, for the N points of the 2P base clouds,
// the per-point data that does not depend on alpha_rot / beta_transl and the UNWEIGHTED
// SE(3) rows (alpha = beta = 1: [R | q] as stored by store_frame_rows).  k_sweep_expand turns
// that into a batch of g variants in one pass:
//   rows     every point's weighted rows for all g variants: al * R, be * q, the (float)
//            casts and a cf target's f32 translation from the raw point -- the arithmetic of
//            the frame kernels' epilogue (k_lrf8.hip, k_knn.hip, k_knn_big.hip), so a row is
//            bitwise what a setup run with that variant's weights stores (1.0 * x == x);
//            and the 3-D trees' (x, y, z, 0) records of the replicas;
//   columns  the SoA columns of replicas 1 .. g-1 (xyz64, xyz32, nrm64, conf64, cloud_of and
//            the 3-D trees' perm, pos, tvec, tvec64), replica v at slot offset v * N;
//   boxes    the 3-D trees' node boxes of the replica clouds;
//   tables   CloudDev / CloudSetup of every virtual cloud (the variant's alpha, beta and
//            cf_target; the normalization fields as the device computed them) and the
//            normalization scale of every virtual pair.
// A streaming kernel: 16-byte stores throughout, 16-byte loads wherever source and
// destination share their alignment (rows, records, boxes always; columns when v * N is a
// multiple of the vector length -- otherwise the column chunk is read element-wise, from
// lines the first replica's pass brought into the L2, and stored as one aligned vector).
// Clouds have odd sizes, so a replica's column segment starts and ends inside a 16-byte
// chunk in general: the first and last chunk of a segment store their covered elements
// one by one.  No atomics, no LDS; the grid is sized from the point count.
#include <hip/hip_runtime.h>

#include "devmath.hpp"
#include "sweep.hpp"
#include "view.hpp"

namespace se3icp {

namespace {

template <class T> struct Vec16;
template <> struct Vec16<double> { using type = double2; };
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<int32_t> { using type = int4; };

// Destination chunk j (16 B, aligned) of the segment col[shift .. shift + n) <- col[0 .. n) + add.
template <class T>
__device__ __forceinline__ void copy_chunk(T* col, int64_t shift, int n, int64_t j, T add) {
    constexpr int E = 16 / (int)sizeof(T);
    using V = typename Vec16<T>::type;
    const int64_t d0 = (shift / E + j) * E;  // first destination element of the chunk
    if (d0 >= shift + n) return;
    const int64_t s0 = d0 - shift;           // its source element (negative in a ragged head)
    T e[E];
    if (s0 >= 0 && s0 + E <= n) {
        if (shift % E == 0) {
            const V x = *reinterpret_cast<const V*>(col + s0);
            const T* px = reinterpret_cast<const T*>(&x);
#pragma unroll
            for (int k = 0; k < E; ++k) e[k] = px[k] + add;
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) e[k] = col[s0 + k] + add;
        }
        V out;
        T* po = reinterpret_cast<T*>(&out);
#pragma unroll
        for (int k = 0; k < E; ++k) po[k] = e[k];
        *reinterpret_cast<V*>(col + d0) = out;
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (s0 + k >= 0 && s0 + k < n) col[d0 + k] = col[s0 + k] + add;
    }
}

__global__ __launch_bounds__(kBlock) void k_sweep_expand(View v, SweepArgs a, int nb_rows, int nb_cols, int nb_box) {
    const int n = a.n, g = a.g;
    int b = blockIdx.x;
    // ---- rows
    if (b < nb_rows) {
        const int i = b * kBlock + (int)threadIdx.x;
        if (i >= n) return;
        if (g > 1) {
            const double2* rec = reinterpret_cast<const double2*>(a.tpt64 + i);
            const double2 r0 = rec[0], r1 = rec[1];
            for (int k = 1; k < g; ++k) {
                double2* o = reinterpret_cast<double2*>(a.tpt64 + (size_t)k * n + i);
                o[0] = r0;
                o[1] = r1;
            }
        }
        if (!a.frames) return;
        const double2* raw = reinterpret_cast<const double2*>(a.raw + (size_t)i * 12);
        double r[12];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double2 x = raw[k];
            r[2 * k] = x.x;
            r[2 * k + 1] = x.y;
        }
        const bool cf_target = a.cf != 0 && v.setup[v.cloud_of[i]].is_target != 0;
        for (int k = 0; k < g; ++k) {
            const double al = a.w[k].alpha, be = a.w[k].beta;
            const double f12[12] = {al * r[0], al * r[1], al * r[2], al * r[3], al * r[4],  al * r[5],
                                    al * r[6], al * r[7], al * r[8], be * r[9], be * r[10], be * r[11]};
            store_frame_rows(v.fr64, v.fr32, k * n + i, f12, cf_target, r[9], r[10], r[11]);
        }
        return;
    }
    b -= nb_rows;
    // ---- columns of replica 1 + b / nb_cols
    if (b < nb_cols * (g - 1)) {
        const int k = 1 + b / nb_cols;
        const int64_t j = (int64_t)(b % nb_cols) * kBlock + threadIdx.x;
        const int64_t shift = (int64_t)k * n;
        const size_t ld = (size_t)v.ld;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            copy_chunk<double>(v.xyz64 + d * ld, shift, n, j, 0.0);
            copy_chunk<double>(v.nrm64 + d * ld, shift, n, j, 0.0);
            copy_chunk<double>(a.tvec64_3 + d * ld, shift, n, j, 0.0);
            copy_chunk<float>(v.xyz32 + d * ld, shift, n, j, 0.f);
            copy_chunk<float>(a.tvec3 + d * ld, shift, n, j, 0.f);
        }
        copy_chunk<double>(v.conf64, shift, n, j, 0.0);
        copy_chunk<int32_t>(a.perm3, shift, n, j, 0);
        copy_chunk<int32_t>(a.pos3, shift, n, j, 0);
        copy_chunk<int32_t>(v.cloud_of, shift, n, j, k * a.nclouds);
        return;
    }
    b -= nb_cols * (g - 1);
    // ---- node boxes of the replica clouds ([nclouds][nnodes][3] f32, a multiple of four)
    if (b < nb_box) {
        const size_t per = (size_t)a.nclouds * a.nnodes3 * 3;  // floats of the base clouds
        const size_t q = (size_t)b * kBlock + threadIdx.x;
        if (4 * q >= per) return;
        const float4 lo = reinterpret_cast<const float4*>(a.lo3)[q];
        const float4 hi = reinterpret_cast<const float4*>(a.hi3)[q];
        for (int k = 1; k < g; ++k) {
            reinterpret_cast<float4*>(a.lo3 + (size_t)k * per)[q] = lo;
            reinterpret_cast<float4*>(a.hi3 + (size_t)k * per)[q] = hi;
        }
        return;
    }
    // ---- tables (one block).  A base entry's alpha, beta and cf_target are rewritten here
    // (variant 0) while the entries of its replicas are built, so those three are never read.
    const int P = a.nclouds / 2;
    for (int t = (int)threadIdx.x; t < g * a.nclouds; t += kBlock) {
        const int k = t / a.nclouds, c = t % a.nclouds;
        const CloudSetup* base = v.setup + c;
        CloudSetup* st = v.setup + t;
        const int32_t is_target = base->is_target;
        if (k > 0) {
            st->k_knn = base->k_knn;
            st->k_lrf = base->k_lrf;
            st->k_nrm = base->k_nrm;
            st->want_cov = base->want_cov;
            st->want_conf = base->want_conf;
            st->is_target = is_target;
            st->_pad = 0;
            for (int x = 0; x < 3; ++x) {
                st->norm_center[x] = base->norm_center[x];
                st->f32_center[x] = base->f32_center[x];
            }
            st->norm_scale = base->norm_scale;
            const CloudDev cb = v.clouds[c];
            v.clouds[t] = CloudDev{cb.off + k * n, cb.n};
            if (a.scales && (c & 1) == 0) a.scales[(size_t)k * P + (c >> 1)] = a.scales[c >> 1];
        }
        st->alpha = a.w[k].alpha;
        st->beta = a.w[k].beta;
        st->cf_target = (a.cf != 0 && is_target != 0) ? 1 : 0;
    }
}

}  // namespace

void launch_sweep_expand(const View& v, const SweepArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.g <= 0) return;
    const int nb_rows = (a.n + kBlock - 1) / kBlock;
    // 16-B chunks a column segment of n elements can touch: n / E + 2 at most (E = 2 for f64)
    const int nb_cols = a.g > 1 ? (a.n / 2 + 2 + kBlock - 1) / kBlock : 0;
    const size_t box4 = (size_t)a.nclouds * a.nnodes3 * 3 / 4;
    const int nb_box = a.g > 1 ? (int)((box4 + kBlock - 1) / kBlock) : 0;
    const int nb = nb_rows + nb_cols * (a.g - 1) + nb_box + 1;
    hipLaunchKernelGGL(k_sweep_expand, dim3(nb), dim3(kBlock), 0, s, v, a, nb_rows, nb_cols, nb_box);
}

}  // namespace se3icp
