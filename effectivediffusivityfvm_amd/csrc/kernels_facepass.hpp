// kernels_facepass.hpp -- the face walk of the gradient passes: g[p] = a sum of one term per face of cell p, from D and one or
// two more planes, in one streaming pass (gfx950, wave64, FP64; nothing like it in the reference).  face_pass<P> is the walk,
// written once; a policy P says what a face and a wall contribute and what is done with the cell's sum:
//   SensPass   the Deff gradient dDeff_raw / dD from (x, D)              k_sens, and k_sens3 on a volume (FpVolume)
//   VjpPass    the field adjoint's dL/dD from (x, lambda, D)             k_vjp
//   TanPass    the field tangent's right-hand side from (x, dD, D)       k_tan
//   HvpPass    the Deff Hessian-vector product from (x, dx, dD, D)       k_hvp
//   FieldHvpPass  the field adjoint's second order from (x, lambda, dx, dlambda, dD, D)   k_fhvp
// All kernels are this one text, so the order of operations per cell, the launch geometry and the order of the final sum are
// the same by construction.
//
// Per cell p, one term per face (weights as the assembly's, fvm_row.hpp: W / E faces carry wx = dy / dx, N / S faces
// wy = dx / dy, a wall ww = dy / (dx / 2)).  The chain rule through the harmonic mean H = 2 Dp Dq / (Dp + Dq) is local:
// dH / dDp = 2 (Dq / (Dp + Dq))^2.  With v[k] = a cell's own value of plane k:
//   interior face to q   s = Dp + Dq;  tq = (s == 0) ? 0 : Dq / s;  tp likewise with Dp;  P::face(p, q, w, tq, tp, cp, cq)
//   left / right wall    e = xp - CL (CR);  c = ww * P::wall(e, v)
//   no face (an image's first and last row)   c = +0.0
//   g[p] = P::finish(((cW + cE) + cN) + cS),  and g[p] = 0 where D[p] == 0.  The pad column of an odd mesh width gets 0.
// A face is evaluated ONCE and gives the term of both its cells with one division each (fp_face): P::face sees both cells
// and both quotients.  The gradient passes' term is (2.0 * (t * t)) * (w * pair(d)) with d[k] = the difference of plane k
// across the face, a value that is the same from either cell (fp_pair_face); the tangent's is antisymmetric (TanPass).
//
// The second output, sum[img] = sum over the image's cells of P::term(cell p, g[p]) -- D[p] * g[p] for the gradient passes, the
// Euler sum -- is a check that needs no reference (each policy says what it equals).  ORDER of that sum: a lane adds its
// cells top to bottom through its work item (first cell of its pair, then the second), the 64 lane sums of a wave are combined by wave_reduce.hpp's fixed DPP tree (row_shr 1, 2, 3, 4, 8, then
// row_bcast 15 and 31: lane 63 holds the sum), and the final kernel (partials_sum_body, one workgroup of 16 waves per image)
// has thread t add the work items' sums t, t + 1024, ... in that order, the same tree per wave, and thread 0 the 16 wave sums
// in wave order.  The order depends on the launch geometry only: the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_reduce.hpp"

namespace deff {

constexpr int FP_ROWS = 8;                       // rows per tile
constexpr int FP_COLS = 128;                     // columns per strip: 2 per lane
template <bool V> struct FpTag { static constexpr bool value = V; };

// The mesh the walk runs on.  FpImage: images of ny rows, four faces per cell.  FpVolume: ONE tall image of ny rows that is a
// volume's slices of `sy` rows one after the other (nz = ny / sy), six faces per cell: rows r - sy and r + sy hold the back
// and front neighbours (weight wz), and a slice's first and last row have no face above / below.
struct FpImage { static constexpr bool VOLUME = false; };
struct FpVolume {
    static constexpr bool VOLUME = true;
    int sy;                                      // rows per slice
    double wz;                                   // dx * dy / dz
};

// what a lane holds of one row: two cells (.x = a, .y = b) of D and of the policy's planes; and one cell of it
template <int NF> struct FpRow { double2 v[NF], D; };
template <int NF> struct FpCell { double v[NF], D; };

// The face of the gradient passes: P::pair(d) of the planes' differences is one value for both cells.
template <class P>
__device__ __forceinline__ void fp_pair_face(const FpCell<P::NF> &p, const FpCell<P::NF> &q, double w, double tq, double tp,
                                             double &cp, double &cq)
{
    double d[P::NF];
#pragma unroll
    for (int k = 0; k < P::NF; ++k) d[k] = p.v[k] - q.v[k];
    const double wd = w * P::pair(d);
    cp = (2.0 * (tq * tq)) * wd;
    cq = (2.0 * (tp * tp)) * wd;
}

// The Deff gradient (k_sens).  The system is self-adjoint: Deff_raw = 2E / (CR - CL)^2 with E = 1/2 sum over faces of
// g_f (dx_f)^2 (the two wall half-faces included), and at the solution dDeff_raw / dg_f = (dx_f)^2 / (CR - CL)^2.  So with
// e = xp - xq a face gives w * (e * e), a wall ww * (e * e), and g[p] = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL));
// g[p] = 0 where D[p] == 0 because the field there is CG's 0, not a limit.  (-e)(-e) = e e: one value per face.
// tests/sensitivity_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
// euler[img] equals Deff_raw of the exact solution (Deff is homogeneous of degree 1 in D: Euler's identity).
// Byte model: x, D read and g written, 24 B per cell.
struct SensPass {
    static constexpr int NF = 1;                 // planes besides D: x
    double den;                                  // (CR - CL) * (CR - CL)
    __device__ __forceinline__ static double pair(const double (&d)[1]) { return d[0] * d[0]; }
    __device__ __forceinline__ static void face(const FpCell<1> &p, const FpCell<1> &q, double w, double tq, double tp, double &cp,
                                                double &cq)
    {
        fp_pair_face<SensPass>(p, q, w, tq, tp, cp, cq);
    }
    __device__ __forceinline__ static double wall(double e, const double (&)[1]) { return e * e; }
    __device__ __forceinline__ double finish(double s) const { return s / den; }
    __device__ __forceinline__ static double term(const FpCell<1> &c, double g) { return c.D * g; }
};

// The field adjoint's pass (k_vjp), planes x and l with A l = dL/dx.  dL/dD[p] = -l^T (dA/dD[p] x - db/dD[p]), and over faces
// l^T (A x - b) = sum over faces a_f (x_p - x_q)(l_p - l_q) + sum over wall cells c_p (x_p - C_wall) l_p.  So with e = xp - xq,
// f = lp - lq a face gives w * (e * f), a wall ww * (e * lp), and g[p] = -(((cW + cE) + cN) + cS).  e and f both change sign
// exactly when the face is seen from its other cell, so e * f has the same value from either side (a zero may differ in sign,
// which no comparison of doubles sees): one division per cell and face for t, four FP64 divisions per cell and no final one.
// tests/field_vjp_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
// euler[img] is -l^T (A x - b): 0 for a converged x whatever l is (A and b are homogeneous of degree 1 in D).
// Byte model: x, l, D read and g written, 32 B per cell.
struct VjpPass {
    static constexpr int NF = 2;                 // planes besides D: x, lambda
    __device__ __forceinline__ static double pair(const double (&d)[2]) { return d[0] * d[1]; }
    __device__ __forceinline__ static void face(const FpCell<2> &p, const FpCell<2> &q, double w, double tq, double tp, double &cp,
                                                double &cq)
    {
        fp_pair_face<VjpPass>(p, q, w, tq, tp, cp, cq);
    }
    __device__ __forceinline__ static double wall(double e, const double (&v)[2]) { return e * v[1]; }
    __device__ __forceinline__ double finish(double s) const { return -s; }
    __device__ __forceinline__ static double term(const FpCell<2> &c, double g) { return c.D * g; }
};

// The field tangent's right-hand side (k_tan), planes x and dD: for A(D) x = b(D) and a direction dD, A dx = db - dA x =: r.
// Over the faces of cell p, (dA x - db)[p] = sum over faces da_f (x_p - x_q) + ww dD_p (x_p - C_wall), and da_f = w dH with
// dH = 2 (Dq / s)^2 dD_p + 2 (Dp / s)^2 dD_q.  With d[p] = (D[p] == 0) ? 0 : dD[p] (a cell that cannot diffuse has no
// direction), e = xp - xq:
//   interior face   h = (2.0 * (tq * tq)) * dp + (2.0 * (tp * tp)) * dq;   c = w * (h * e)
//   wall            c = ww * (dp * (xp - CL (CR)))
//   r[p] = -(((cW + cE) + cN) + cS).
// h has the same bits seen from either cell (the two products change places and the addition commutes) and e changes sign
// exactly, so the other cell's term is -c: one evaluation per face, as in the gradient passes.
// tests/tangent_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
// sum[img] is the squared norm of r: for dD = D it is that of the forward residual b - A x (x is of degree 0 in D).
// Byte model: x, dD, D read and r written, 32 B per cell.
struct TanPass {
    static constexpr int NF = 2;                 // planes besides D: x, dD
    __device__ __forceinline__ static void face(const FpCell<2> &p, const FpCell<2> &q, double w, double tq, double tp, double &cp,
                                                double &cq)
    {
        const double dp = (p.D == 0) ? 0 : p.v[1], dq = (q.D == 0) ? 0 : q.v[1];
        const double h = (2.0 * (tq * tq)) * dp + (2.0 * (tp * tp)) * dq;
        cp = w * (h * (p.v[0] - q.v[0]));
        cq = -cp;
    }
    // (the wall cell's own D == 0 needs no test here: the walk sets its r to 0)
    __device__ __forceinline__ static double wall(double e, const double (&v)[2]) { return v[1] * e; }
    __device__ __forceinline__ double finish(double s) const { return -s; }
    __device__ __forceinline__ static double term(const FpCell<2> &, double g) { return g * g; }
};

// The Deff Hessian-vector product (k_hvp), planes x, y = dx (the field tangent along dD) and dD.  g = dDeff_raw / dD is
// SensPass's map, a function of (x, D), so H dD = dg/dD . dD + dg/dx . dx.  Both parts are face-local: a face gives cell p
// (2 tq^2) w e^2 with tq = Dq / s, and along dD the quotient moves by u = (tp dq - tq dp) / s, the difference e by f = yp - yq.
// With d[p] = (D[p] == 0) ? 0 : dD[p] (a cell that cannot diffuse has no direction):
//   interior face   u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;  e = xp - xq;  f = yp - yq;
//                   c = w * ((4.0 * tq) * (u * (e * e)) + (4.0 * (tq * tq)) * (e * f))
//   wall            e = xp - CL (CR);  c = ww * (2.0 * (e * yp))
//   hv[p] = (((cW + cE) + cN) + cS) / ((CR - CL) * (CR - CL)),  hv[p] = 0 where D[p] == 0.
// Seen from q, u is exactly -u (the two products change places in a subtraction) and e * e, e * f have the same bits (both
// factors change sign exactly; a zero may differ in sign, which no comparison of doubles sees), so
//   cq = w * ((4.0 * tp) * ((-u) * (e * e)) + (4.0 * (tp * tp)) * (e * f)):
// one evaluation per face, three FP64 divisions per face (tq, tp, u) where the other policies have two.
// tests/sens_hvp_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
// sum[img] = sum of d[p] * hv[p] = dD^T H dD, the curvature of Deff_raw along dD: never positive at a converged field with
// its own tangent (Deff is a minimum over fields of functions linear in D, hence concave).
// Byte model: x, dx, dD, D read and hv written, 40 B per cell.
struct HvpPass {
    static constexpr int NF = 3;                 // planes besides D: x, dx, dD
    double den;                                  // (CR - CL) * (CR - CL)
    __device__ __forceinline__ static void face(const FpCell<3> &p, const FpCell<3> &q, double w, double tq, double tp, double &cp,
                                                double &cq)
    {
        const double s = p.D + q.D;
        const double dp = (p.D == 0) ? 0 : p.v[2], dq = (q.D == 0) ? 0 : q.v[2];
        const double u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;
        const double e = p.v[0] - q.v[0], f = p.v[1] - q.v[1];
        const double ee = e * e, ef = e * f;
        cp = w * ((4.0 * tq) * (u * ee) + (4.0 * (tq * tq)) * ef);
        cq = w * ((4.0 * tp) * ((-u) * ee) + (4.0 * (tp * tp)) * ef);
    }
    __device__ __forceinline__ static double wall(double e, const double (&v)[3]) { return 2.0 * (e * v[1]); }
    __device__ __forceinline__ double finish(double s) const { return s / den; }
    __device__ __forceinline__ static double term(const FpCell<3> &c, double g) { return ((c.D == 0) ? 0 : c.v[2]) * g; }
};

// The second-order field adjoint (k_fhvp), planes x, l (A l = w), y = dx and m = dl along dD, and dD.  g = grad of w^T x(D) is
// VjpPass's map, a function of (x, l, D) with w held fixed, so S_w dD = dg/dD . dD + dg/dx . y + dg/dl . m: y is the field
// tangent (A y = db - dA x), m the adjoint's (A m = -dA l: TanPass on l with both wall values 0).  All three parts are
// face-local: a face gives cell p (2 tq^2) w e fl, the quotient moves by u as in HvpPass, e by ed, fl by fm.
// With d[p] = (D[p] == 0) ? 0 : dD[p]:
//   interior face   u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;  e = xp - xq;  fl = lp - lq;  ed = yp - yq;  fm = mp - mq;
//                   ef = e * fl;  k = ed * fl + e * fm;
//                   c = w * ((4.0 * tq) * (u * ef) + (2.0 * (tq * tq)) * k)
//   wall            e = xp - CL (CR);  c = ww * (yp * lp + e * mp)
//   hv[p] = -(((cW + cE) + cN) + cS),  hv[p] = 0 where D[p] == 0.
// Seen from q, u is exactly -u and ef, k have the same bits (every difference changes sign exactly, so each product keeps
// its bits and the addition its operands; a zero may differ in sign), so
//   cq = w * ((4.0 * tp) * ((-u) * ef) + (2.0 * (tp * tp)) * k):
// one evaluation per face, three FP64 divisions per face as in HvpPass.
// tests/field_hvp_model.py states the same expressions in numpy, in this order: the map is compared bit for bit.
// sum[img] = sum of d[p] * hv[p] = dD^T S_w dD.  It has no sign; w^T x is homogeneous of degree 0 in D, so S_w D = -g.
// Byte model: x, l, dx, dl, dD, D read and hv written, 56 B per cell.
struct FieldHvpPass {
    static constexpr int NF = 5;                 // planes besides D: x, lambda, dx, dlambda, dD
    __device__ __forceinline__ static void face(const FpCell<5> &p, const FpCell<5> &q, double w, double tq, double tp, double &cp,
                                                double &cq)
    {
        const double s = p.D + q.D;
        const double dp = (p.D == 0) ? 0 : p.v[4], dq = (q.D == 0) ? 0 : q.v[4];
        const double u = (s == 0) ? 0 : (tp * dq - tq * dp) / s;
        const double e = p.v[0] - q.v[0], fl = p.v[1] - q.v[1], ed = p.v[2] - q.v[2], fm = p.v[3] - q.v[3];
        const double ef = e * fl, k = ed * fl + e * fm;
        cp = w * ((4.0 * tq) * (u * ef) + (2.0 * (tq * tq)) * k);
        cq = w * ((4.0 * tp) * ((-u) * ef) + (2.0 * (tp * tp)) * k);
    }
    // (e is plane 0's value against the wall: x)
    __device__ __forceinline__ static double wall(double e, const double (&v)[5]) { return v[2] * v[1] + e * v[3]; }
    __device__ __forceinline__ double finish(double s) const { return -s; }
    __device__ __forceinline__ static double term(const FpCell<5> &c, double g) { return ((c.D == 0) ? 0 : c.v[4]) * g; }
};

template <int NF> __device__ __forceinline__ FpCell<NF> fp_a(const FpRow<NF> &r)
{
    FpCell<NF> c;
#pragma unroll
    for (int k = 0; k < NF; ++k) c.v[k] = r.v[k].x;
    c.D = r.D.x;
    return c;
}
template <int NF> __device__ __forceinline__ FpCell<NF> fp_b(const FpRow<NF> &r)
{
    FpCell<NF> c;
#pragma unroll
    for (int k = 0; k < NF; ++k) c.v[k] = r.v[k].y;
    c.D = r.D.y;
    return c;
}

// One interior face between cells p and q, weight w: cp = the term of p, cq = the term of q.
template <class P>
__device__ __forceinline__ void fp_face(const FpCell<P::NF> &p, const FpCell<P::NF> &q, double w, double &cp, double &cq)
{
    const double s = p.D + q.D;
    const double tq = (s == 0) ? 0 : q.D / s;
    const double tp = (s == 0) ? 0 : p.D / s;
    P::face(p, q, w, tq, tp, cp, cq);
}

__device__ __forceinline__ double fp_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The body of a __global__ __launch_bounds__(256) kernel.  One wave per work item = `kt` consecutive tiles of FP_ROWS rows x 128
// columns of one image (a column strip streamed top to bottom), 4 work items (vertically adjacent) per workgroup; a lane holds
// two cells (a, b) of each row.
//  - Rows of the planes and D pass through a window of three (the row in hand, the one below it for the S faces, the one in
//    flight): the 16-byte loads of row r + 2 are issued before the arithmetic of row r.  Rows are clamped into the image, never
//    tested, and every lane loads (a lane beyond the arrays reads the row's first cells): the count of loads in flight is the
//    same on every path.
//  - A face is evaluated ONCE: per row a lane computes the face a|b, the E face of b and the two S faces.  The W term of a
//    is the other half of the left lane's E face (wave_shr:1); the N terms are the other halves of the S faces of the row
//    above, carried down the strip.  A work item that starts inside an image evaluates the faces above its first row once.
//  - The strip's outer neighbours: per tile, lanes 0...7 load the cell west of the strip for one row each (and the strip's
//    own first cell) and evaluate that face, or the left wall's term; lanes 8...15 load the cell east of it.  A row takes
//    them from there with v_readlane: lane 0's W term and lane 63's E neighbour enter as the `old` operand of the lane
//    shifts, no per-row selects.  The next tile's outer cells are loaded a tile ahead -- with three planes or more (HvpPass, FieldHvpPass) into the
//    same registers during the tile's last row, once that row has taken its own: a second set would cost 16 VGPRs and the
//    fourth wave per SIMD.
//  - Only the last strip (EDGE) knows the right wall, the cells beyond it and the pad column, by per-lane selects.
// Addresses are 64-bit (image base + row base are wave-uniform, the lane adds its column).  No LDS, no waiting.
// On a volume (M = FpVolume; the 2-D kernels compile none of it):
//  - slice borders inside the tall image: the N term carried down the strip is +0.0 into a slice's first row, the S term
//    +0.0 in its last, and an item that starts on a slice's first row has nothing above it.  The row's place in its slice is
//    a counter, wave-uniform like the row; items and tiles may straddle borders, several of them with sy < 8.
//  - the B and F terms: each z face is evaluated from the cell's own side (P::face's term of p; the quotient and the term of q
//    are dead code), one division per cell and face as everywhere -- a face evaluated once would have to be carried across
//    sy rows.  Rows r - sy and r + sy are loaded like the window's own, a row ahead and clamped into the image, and a term
//    from outside the volume (the first / last slice) is zeroed afterwards.  g[p] = P::finish(((((cW + cE) + cN) + cS) + cB) + cF).
// partial[img * per_img + tx * cpi + chunk] = the work item's sum of P::term (cpi = work items per strip and image).
template <class P, class M = FpImage>
__device__ __forceinline__ void face_pass(const P &pol, const double *const (&planes)[P::NF], const double *D, int nx, int nxt,
                                          int ny, int nimg, int ntx, int cpi, int kt, double wx, double wy, double ww, double CL,
                                          double CR, double *g, double *partial, const M mesh = M{})
{
    constexpr bool VOL = M::VOLUME;
    constexpr int NF = P::NF;
    using Row = FpRow<NF>;
    using Cell = FpCell<NF>;
    constexpr bool OUTER_IN_PLACE = NF >= 3;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t gy = (size_t)nimg * (size_t)cpi;
    const size_t wt = (size_t)blockIdx.x * 4u + (size_t)wave;
    if (wt >= (size_t)ntx * gy) return;
    const int tx = (int)(wt / gy);
    const size_t ty = wt % gy;
    const int img = (int)(ty / (size_t)cpi), chunk = (int)(ty - (size_t)img * (size_t)cpi);
    const int l_begin = chunk * FP_ROWS * kt;                    // rows [l_begin, l_end) of the image
    const int l_end = min(l_begin + FP_ROWS * kt, ny);
    const int col0 = tx * FP_COLS, col = col0 + 2 * lane;
    const size_t ibase = (size_t)img * (size_t)ny * (size_t)nx;
    const double *vi[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) vi[k] = planes[k] + ibase;
    const double *Di = D + ibase;
    double *gi = g + ibase;

    auto run = [&](auto edge_tag) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        const bool va = !EDGE || col < nxt, vb = !EDGE || col + 1 < nxt;        // cells of the mesh
        const bool a_last = EDGE && col == nxt - 1, b_last = EDGE && col + 1 == nxt - 1;
        const bool st = !EDGE || col < nx;                                       // lanes inside the arrays
        const int colx = st ? col : 0;
        auto load_row = [&](int li, Row &r) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(max(li, 0), ny - 1) * (size_t)nx;      // wave-uniform clamp
#pragma unroll
            for (int k = 0; k < NF; ++k) r.v[k] = *reinterpret_cast<const double2 *>(vi[k] + rb + colx);
            r.D = *reinterpret_cast<const double2 *>(Di + rb + colx);
        };
        // outer cells of a tile: lane h < 8 row l + h west of the strip, lane 8 + h row l + h east of it; lanes above 15 repeat lane 15
        const int hl = min(lane, 15), hq = hl & 7;
        const bool wwall = tx == 0;
        const int hcol = hl < 8 ? (wwall ? 0 : col0 - 1) : (col0 + FP_COLS < nxt ? col0 + FP_COLS : 0);
        struct Outer { Cell h, a; };                                             // the cell outside, the strip's own first cell
        auto load_outer = [&](int l, Outer &o) __attribute__((always_inline)) {
            const size_t rb = (size_t)min(l + hq, ny - 1) * (size_t)nx;
#pragma unroll
            for (int k = 0; k < NF; ++k) o.h.v[k] = vi[k][rb + hcol];
            o.h.D = Di[rb + hcol];
#pragma unroll
            for (int k = 0; k < NF; ++k) o.a.v[k] = vi[k][rb + col0];
            o.a.D = Di[rb + col0];
        };

        // a volume's rows li - sy and li + sy, back and front of row li
        auto load_z = [&](int li, Row &b, Row &t) __attribute__((always_inline)) {
            if constexpr (VOL) {
                load_row(li - mesh.sy, b);
                load_row(li + mesh.sy, t);
            }
        };
        Row c, n, f;                                             // the row in hand, the next, the one in flight
        Row zb, zf, zb2, zf2;                                    // a volume: back and front of the row in hand, and of the next in flight
        Outer o, o2;
        load_row(l_begin - 1, f);
        load_row(l_begin, c);
        load_row(l_begin + 1, n);
        load_z(l_begin, zb, zf);
        load_outer(l_begin, o);
        int rs = 0;                                              // a volume: the row's place in its slice
        if constexpr (VOL) rs = l_begin % mesh.sy;
        // the N terms of the item's first row: the faces above it (nothing above an image's first row)
        double nA, nB, unused;
        fp_face<P>(fp_a(f), fp_a(c), wy, unused, nA);
        fp_face<P>(fp_b(f), fp_b(c), wy, unused, nB);
        if (VOL ? rs == 0 : l_begin == 0) { nA = 0.0; nB = 0.0; }
        double acc = 0.0;
#pragma unroll 1
        for (int l = l_begin; l < l_end; l += FP_ROWS) {
            if constexpr (!OUTER_IN_PLACE) load_outer(l + FP_ROWS, o2);
            double hw;                                           // lanes 0...7: the W term of the strip's first cell in row l + lane
            if (wwall) hw = ww * P::wall(o.a.v[0] - CL, o.a.v);
            else fp_face<P>(o.a, o.h, wx, hw, unused);
#pragma unroll
            for (int q = 0; q < FP_ROWS; ++q) {
                const int r = l + q;
                if (r >= l_end) break;                           // wave-uniform: the item's (or the image's) last rows
                load_row(r + 2, f);
                load_z(r + 1, zb2, zf2);
                const double hwq = fp_readlane(hw, q);
                const Cell ca = fp_a(c), cb = fp_b(c);
                Cell ce;                                         // the next lane's a; lane 63 keeps the cell east of the strip
#pragma unroll
                for (int k = 0; k < NF; ++k) ce.v[k] = dpp_f64_keep<0x130>(ca.v[k], fp_readlane(o.h.v[k], 8 + q));   // wave_shl:1
                ce.D = dpp_f64_keep<0x130>(ca.D, fp_readlane(o.h.D, 8 + q));
                if constexpr (OUTER_IN_PLACE) {
                    if (q == FP_ROWS - 1) load_outer(l + FP_ROWS, o);
                }
                double mA, mB, eB, eQ, sA, sB, nA2, nB2;
                fp_face<P>(ca, cb, wx, mA, mB);                      // a | b
                fp_face<P>(cb, ce, wx, eB, eQ);                      // b | the next lane's a
                if constexpr (EDGE) {                                // the right wall
                    const double wa = ww * P::wall(ca.v[0] - CR, ca.v), wb = ww * P::wall(cb.v[0] - CR, cb.v);
                    if (a_last) mA = wa;
                    if (b_last) eB = wb;
                }
                const double wA = dpp_f64_keep<0x138>(eQ, hwq);      // wave_shr:1, lane 0 keeps the strip's outer W term
                fp_face<P>(ca, fp_a(n), wy, sA, nA2);
                fp_face<P>(cb, fp_b(n), wy, sB, nB2);
                double ga, gb;
                if constexpr (VOL) {
                    if (rs == mesh.sy - 1) { sA = 0.0; sB = 0.0; nA2 = 0.0; nB2 = 0.0; }   // wave-uniform: a slice's last row
                    rs = rs == mesh.sy - 1 ? 0 : rs + 1;
                    double bA, bB, fA, fB;
                    fp_face<P>(ca, fp_a(zb), mesh.wz, bA, unused);
                    fp_face<P>(cb, fp_b(zb), mesh.wz, bB, unused);
                    fp_face<P>(ca, fp_a(zf), mesh.wz, fA, unused);
                    fp_face<P>(cb, fp_b(zf), mesh.wz, fB, unused);
                    if (r < mesh.sy) { bA = 0.0; bB = 0.0; }                 // wave-uniform: the first slice, the last
                    if (r >= ny - mesh.sy) { fA = 0.0; fB = 0.0; }
                    ga = pol.finish(((((wA + mA) + nA) + sA) + bA) + fA);
                    gb = pol.finish(((((mB + eB) + nB) + sB) + bB) + fB);
                    zb = zb2; zf = zf2;
                } else {
                    if (r == ny - 1) { sA = 0.0; sB = 0.0; }         // wave-uniform
                    ga = pol.finish(((wA + mA) + nA) + sA);
                    gb = pol.finish(((mB + eB) + nB) + sB);
                }
                if (!va || ca.D == 0) ga = 0.0;
                if (!vb || cb.D == 0) gb = 0.0;
                if (va) acc += P::term(ca, ga);
                if (vb) acc += P::term(cb, gb);
                if (st) *reinterpret_cast<double2 *>(gi + (size_t)r * (size_t)nx + col) = make_double2(ga, gb);
                nA = nA2; nB = nB2;
                c = n; n = f;
            }
            if constexpr (!OUTER_IN_PLACE) o = o2;
        }
        const double s = wave_sum_to_lane63(acc);
        if (lane == 63) partial[(size_t)img * ((size_t)ntx * cpi) + (size_t)tx * cpi + chunk] = s;
    };
    if (tx == ntx - 1) run(FpTag<true>{});
    else run(FpTag<false>{});
}

}  // namespace deff
