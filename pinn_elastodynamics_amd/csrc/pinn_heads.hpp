// The residual heads' formulas, once per family: residuals of the network's output streams, and the adjoint seeds dL/dY from
// g_i = dL/df_i.  chain_kernel (pinn_device.hpp), fp32_chain_kernel (pinn_fp32.hpp) and Fused::fwd_head (pinn_fused.hpp) all call
// these; the Python mirrors are the model classes and oracle/.
//
// Everything here is a __device__ __forceinline__ template that touches no memory: what a head reads from `aux` (the plate's frozen
// streams, a traction set's normals and targets) is loaded by the kernel and handed in -- with the loads in here the compiler schedules
// them differently and the fused kernels' device code moves (profiles/heads_single_source_isa.txt).  The outputs are read through a
// callable Y(s, o) -- stream s of output o -- and the seeds are written through a callable adj(s, o) that returns a reference, so that
// one definition serves the layouts Y[s][nb][o] of chain_kernel and Y[s][o] of the other two.  `a` is the kernel's argument struct:
// only its c1, c2, G, rho are read.  A seed function writes the non-zero seeds only: the caller zeroes adj first.
// Written out at their sites instead, each for a measured reason (profiles/heads_single_source_isa.txt, _ab.txt): set kinds 1 and 2 of
// Fused::fwd_head (through the calls a one-stream fused kernel's device code moves); HEAD_PLATE and HEAD_MATERIAL3D of chain_kernel (their
// register spills move in one instantiation each); the four plate heads of fp32_chain_kernel (on gfx950 the compiler contracts the
// plate's expressions into other fused multiply-adds when they sit in these functions, and the plate's fp32 outputs change in the last bits).
//
// What stays with the kernel: the mask of padded points, the term weights (g_i = 2 tw_i f_i [vm]), where the squares go (fp32 loss
// sums, a score, fp64 moment sums), and the guards of the lanes that write.
//
// The expressions are bit-for-bit part of the contract (the parity tests compare kernels that share them): keep the association
// and the order of the additions when editing.
#pragma once
#include <hip/hip_runtime.h>

namespace pinn {
namespace heads {

struct Strains2 { float e11, e22, e12; };                      // INF:216-218
struct Strains3 { float e11, e22, e33, e12, e13, e23; };

// ---- wave family: net_f_sig INF:221-265; outputs (u,v,ut,vt,s11,s22,s12); streams (value, d/dx, d/dy, d/dt)
template <class YF>
__device__ __forceinline__ Strains2 wave_strains(YF Y) {
    return {Y(1, 0), Y(2, 1), Y(2, 0) + Y(1, 1)};                           // INF:216-218
}

template <class A, class YF>
__device__ __forceinline__ void wave_residuals(const A& a, YF Y, float (&f)[7]) {
    const float e11 = Y(1, 0), e22 = Y(2, 1), e12 = Y(2, 0) + Y(1, 1);      // (wave_strains)
    f[0] = Y(1, 4) + Y(2, 6) - a.rho * Y(3, 2);                             // f_u   INF:262
    f[1] = Y(2, 5) + Y(1, 6) - a.rho * Y(3, 3);                             // f_v   INF:263
    f[2] = Y(3, 0) - Y(0, 2);                                               // f_ut  INF:248
    f[3] = Y(3, 1) - Y(0, 3);                                               // f_vt  INF:249
    f[4] = Y(0, 4) - (a.c1 * e11 + a.c2 * e22);                             // f_s11 INF:244
    f[5] = Y(0, 5) - (a.c2 * e11 + a.c1 * e22);                             // f_s22 INF:246
    f[6] = Y(0, 6) - a.G * e12;                                             // f_s12 INF:245
}

template <class A, class AF>
__device__ __forceinline__ void wave_seeds(const A& a, const float (&g)[7], AF adj) {
    adj(0, 2) = -g[2];
    adj(0, 3) = -g[3];
    adj(0, 4) = g[4];
    adj(0, 5) = g[5];
    adj(0, 6) = g[6];
    adj(1, 0) = -a.c1 * g[4] - a.c2 * g[5];
    adj(1, 1) = -a.G * g[6];
    adj(1, 4) = g[0];
    adj(1, 6) = g[1];
    adj(2, 0) = -a.G * g[6];
    adj(2, 1) = -a.c2 * g[4] - a.c1 * g[5];
    adj(2, 5) = g[1];
    adj(2, 6) = g[0];
    adj(3, 0) = g[2];
    adj(3, 1) = g[3];
    adj(3, 2) = -a.rho * g[0];
    adj(3, 3) = -a.rho * g[1];
}

// ---- 3-D family: Navier-Cauchy residuals (oracle/nc3d_oracle.py: the 3-D statement of INF:221-265); outputs
// (u,v,w, ut,vt,wt, s11,s22,s33, s12,s13,s23); streams (value, d/dx, d/dy, d/dz, d/dt); c1 = lambda + 2G, c2 = lambda
template <class YF>
__device__ __forceinline__ Strains3 nc3d_strains(YF Y) {
    return {Y(1, 0), Y(2, 1), Y(3, 2), Y(2, 0) + Y(1, 1), Y(3, 0) + Y(1, 2), Y(3, 1) + Y(2, 2)};
}

template <class A, class YF>
__device__ __forceinline__ void nc3d_residuals(const A& a, YF Y, float (&f)[12]) {
    const float e11 = Y(1, 0), e22 = Y(2, 1), e33 = Y(3, 2);
    const float e12 = Y(2, 0) + Y(1, 1), e13 = Y(3, 0) + Y(1, 2), e23 = Y(3, 1) + Y(2, 2);
    f[0] = Y(1, 6) + Y(2, 9) + Y(3, 10) - a.rho * Y(4, 3);
    f[1] = Y(1, 9) + Y(2, 7) + Y(3, 11) - a.rho * Y(4, 4);
    f[2] = Y(1, 10) + Y(2, 11) + Y(3, 8) - a.rho * Y(4, 5);
    f[3] = Y(4, 0) - Y(0, 3);
    f[4] = Y(4, 1) - Y(0, 4);
    f[5] = Y(4, 2) - Y(0, 5);
    f[6] = Y(0, 6) - (a.c1 * e11 + a.c2 * (e22 + e33));
    f[7] = Y(0, 7) - (a.c1 * e22 + a.c2 * (e11 + e33));
    f[8] = Y(0, 8) - (a.c1 * e33 + a.c2 * (e11 + e22));
    f[9] = Y(0, 9) - a.G * e12;
    f[10] = Y(0, 10) - a.G * e13;
    f[11] = Y(0, 11) - a.G * e23;
}

template <class A, class AF>
__device__ __forceinline__ void nc3d_seeds(const A& a, const float (&g)[12], AF adj) {
    // value stream
    adj(0, 3) = -g[3];
    adj(0, 4) = -g[4];
    adj(0, 5) = -g[5];
#pragma unroll
    for (int i = 6; i < 12; ++i) adj(0, i) = g[i];
    // d/dx
    adj(1, 0) = -(a.c1 * g[6] + a.c2 * (g[7] + g[8]));
    adj(1, 1) = -a.G * g[9];
    adj(1, 2) = -a.G * g[10];
    adj(1, 6) = g[0];
    adj(1, 9) = g[1];
    adj(1, 10) = g[2];
    // d/dy
    adj(2, 0) = -a.G * g[9];
    adj(2, 1) = -(a.c1 * g[7] + a.c2 * (g[6] + g[8]));
    adj(2, 2) = -a.G * g[11];
    adj(2, 9) = g[0];
    adj(2, 7) = g[1];
    adj(2, 11) = g[2];
    // d/dz
    adj(3, 0) = -a.G * g[10];
    adj(3, 1) = -a.G * g[11];
    adj(3, 2) = -(a.c1 * g[8] + a.c2 * (g[6] + g[7]));
    adj(3, 10) = g[0];
    adj(3, 11) = g[1];
    adj(3, 8) = g[2];
    // d/dt
    adj(4, 0) = g[3];
    adj(4, 1) = g[4];
    adj(4, 2) = g[5];
    adj(4, 3) = -a.rho * g[0];
    adj(4, 4) = -a.rho * g[1];
    adj(4, 5) = -a.rho * g[2];
}

// ---- plate family: composite F = P + D*N (PLATE:383-387) with product-rule derivatives, then net_f_sig PLATE:404-439; outputs
// (u,v,s11,s22,s12); streams (value, x, y, t, tt); D, P [stream][field]: the point's frozen streams, aux = [D|P][stream][field][n]
// F = P + D*N and its streams by the product rule, F holding P on entry
template <class YF>
__device__ __forceinline__ void plate_composite(YF Y, const float (&D)[5][5], float (&F)[5][5]) {
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        const float n0 = Y(0, o);
        F[0][o] += D[0][o] * n0;
#pragma unroll
        for (int k = 1; k <= 3; ++k) F[k][o] += D[k][o] * n0 + D[0][o] * Y(k, o);
        F[4][o] += D[4][o] * n0 + 2.0f * D[3][o] * Y(3, o) + D[0][o] * Y(4, o);
    }
}

__device__ __forceinline__ Strains2 plate_strains(const float (&F)[5][5]) {
    return {F[1][0], F[2][1], F[2][0] + F[1][1]};
}

template <class A>
__device__ __forceinline__ void plate_residuals(const A& a, const float (&F)[5][5], float (&f)[5]) {
    const float e11 = F[1][0], e22 = F[2][1], e12 = F[2][0] + F[1][1];
    f[0] = F[1][2] + F[2][4] - a.rho * F[4][0];                             // f_u   PLATE:436
    f[1] = F[2][3] + F[1][4] - a.rho * F[4][1];                             // f_v   PLATE:437
    f[2] = F[0][2] - (a.c1 * e11 + a.c2 * e22);                             // f_s11 PLATE:421
    f[3] = F[0][3] - (a.c2 * e11 + a.c1 * e22);                             // f_s22 PLATE:423
    f[4] = F[0][4] - a.G * e12;                                             // f_s12 PLATE:422
}

// seeds of the composite, Fb = dL/dF, taken back through D to the net's own streams (writes outputs 0..4 of all five streams)
template <class A, class AF>
__device__ __forceinline__ void plate_seeds(const A& a, const float (&g)[5], const float (&D)[5][5], AF adj) {
    float Fb[5][5];
#pragma unroll
    for (int st = 0; st < 5; ++st)
#pragma unroll
        for (int o = 0; o < 5; ++o) Fb[st][o] = 0.0f;
    Fb[0][2] = g[2];
    Fb[0][3] = g[3];
    Fb[0][4] = g[4];
    Fb[1][0] = -a.c1 * g[2] - a.c2 * g[3];
    Fb[2][1] = -a.c2 * g[2] - a.c1 * g[3];
    Fb[2][0] = -a.G * g[4];
    Fb[1][1] = -a.G * g[4];
    Fb[1][2] = g[0];
    Fb[2][4] = g[0];
    Fb[4][0] = -a.rho * g[0];
    Fb[2][3] = g[1];
    Fb[1][4] = g[1];
    Fb[4][1] = -a.rho * g[1];
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        adj(0, o) = Fb[0][o] * D[0][o] + Fb[1][o] * D[1][o] + Fb[2][o] * D[2][o] + Fb[3][o] * D[3][o] + Fb[4][o] * D[4][o];
        adj(1, o) = Fb[1][o] * D[0][o];
        adj(2, o) = Fb[2][o] * D[0][o];
        adj(3, o) = Fb[3][o] * D[0][o] + 2.0f * Fb[4][o] * D[3][o];
        adj(4, o) = Fb[4][o] * D[0][o];
    }
}

// ---- traction of the plate's composite on the hole (net_t PLATE:452-461), value stream only: (tx, ty) of F = P0 + D0 N on the normal
// (nx, ny); the point's aux rows are D0[0..4], P0[5..9], nx[10], ny[11]
template <class YF>
__device__ __forceinline__ void plate_traction_residual(YF Y, const float (&D0)[5], const float (&P0)[5], float nx, float ny, float& tx, float& ty) {
    float Fv[5];
#pragma unroll
    for (int o = 0; o < 5; ++o) Fv[o] = P0[o] + D0[o] * Y(0, o);
    tx = Fv[2] * nx + Fv[4] * ny, ty = Fv[4] * nx + Fv[3] * ny;
}

template <class AF>
__device__ __forceinline__ void plate_traction_seeds(float gx, float gy, float nx, float ny, const float (&D0)[5], AF adj) {
    adj(0, 2) = gx * nx * D0[2];
    adj(0, 3) = gy * ny * D0[3];
    adj(0, 4) = (gx * ny + gy * nx) * D0[4];
}

// ---- traction of the wave net's own stresses (outputs 4, 5, 6 = s11, s22, s12) on a boundary with per-point normals, less the
// prescribed traction (net_surf_var INF:267-276); the point's aux rows are nx[0], ny[1], tx[2], ty[3]; normals used as given
// (tx, ty): the stresses' traction vector; the residual is r = t - target, the subtraction left to the kernel next to its load
template <class YF>
__device__ __forceinline__ void wave_traction(YF Y, float nx, float ny, float& tx, float& ty) {
    tx = Y(0, 4) * nx + Y(0, 6) * ny;
    ty = Y(0, 6) * nx + Y(0, 5) * ny;
}

template <class AF>
__device__ __forceinline__ void wave_traction_seeds(float gx, float gy, float nx, float ny, AF adj) {
    adj(0, 4) = gx * nx;
    adj(0, 5) = gy * ny;
    adj(0, 6) = gx * ny + gy * nx;
}

}  // namespace heads
}  // namespace pinn
