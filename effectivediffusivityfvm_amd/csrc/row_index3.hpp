// row_index3.hpp -- the a-priori row table of the native 3-phase system (deff_assemble_3phase_native), host + device: which
// table row a cell gets (k_phase_codes3, kernels_fill.hpp) and which doubles that row holds (build_rows3, from fvm_row like
// build_lut_rows, so they are the very doubles k_assemble_from_D writes).
//
// Row 0 is the zero row (cells outside the mesh), row 1 the identity row of the cells DiscretizeMatrix2D_ImpSolid takes out
// (Grid 1 or 2, cuh:750-752).  An active cell is fluid (0) or gas (2) -- a solid cell is never active --, each neighbour is
// fluid, solid (1) or gas by its pixel alone.  Rows are numbered densely per position class and count only the neighbours
// whose links the class has (fvm_row never reads the others): 2 * 3^4 = 162 interior rows, 2 * 3^3 = 54 for each of the four
// edge classes, 2 * 3^2 = 18 for each corner, 450 in all, 452 with rows 0 and 1 (LUT_MAX_ROWS is 512; 162 rows for every
// class would be 1 458).
#pragma once
#include <cstddef>
#include "fvm_row.hpp"

namespace deff {

constexpr int NATIVE3_IDENTITY = 1;
constexpr int NATIVE3_FIRST = 2;
constexpr int NATIVE3_ROWS = 452;

// links a position class has: W unless first column, E unless last column, S (row + 1) unless last row, N unless first row
__host__ __device__ inline int native3_links(int ycls, int xcls)
{
    return (xcls == POS_INTERIOR ? 2 : 1) + (ycls == POS_INTERIOR ? 2 : 1);
}

__host__ __device__ inline int native3_class_rows(int ycls, int xcls)
{
    int n = 2;
    for (int k = native3_links(ycls, xcls); k > 0; --k) n *= 3;
    return n;
}

// first row of class (ycls, xcls), classes in the order ycls * 3 + xcls
__host__ __device__ inline int native3_class_base(int ycls, int xcls)
{
    int base = NATIVE3_FIRST;
    for (int c = 0; c < ycls * 3 + xcls; ++c) base += native3_class_rows(c / 3, c % 3);
    return base;
}

// own: 0 fluid, 1 gas.  cw / ce / cs / cn: 0 fluid, 1 solid, 2 gas; those of links the class does not have are ignored.
__host__ __device__ inline int native3_row(int ycls, int xcls, int own, int cw, int ce, int cs, int cn)
{
    int idx = own, mul = 2;
    if (xcls != POS_FIRST) { idx += mul * cw; mul *= 3; }
    if (xcls != POS_LAST) { idx += mul * ce; mul *= 3; }
    if (ycls != POS_LAST) { idx += mul * cs; mul *= 3; }
    if (ycls != POS_FIRST) { idx += mul * cn; mul *= 3; }
    return native3_class_base(ycls, xcls) + idx;
}

// pixel -> neighbour class (cuh:1518-1529: > 200 solid, < 50 gas, otherwise fluid)
__host__ __device__ inline int native3_pixel_class(unsigned v) { return v > 200 ? 1 : (v < 50 ? 2 : 0); }

// rows[NATIVE3_ROWS][6] = A0, aW, aE, aS, aN, b.  Tuples that differ only in a neighbour the class has no link to name the
// same row and write the same doubles into it: fvm_row never reads that neighbour.
inline void build_rows3(double *rows, double Ds, double Df, double Dg, double dx, double dy, double CL, double CR)
{
    for (int k = 0; k < NATIVE3_ROWS * 6; ++k) rows[k] = 0.0;
    rows[NATIVE3_IDENTITY * 6] = 1.0;
    const double Dn[3] = {Df, Ds, Dg}, Do[2] = {Df, Dg};
    for (int ycls = 0; ycls < 3; ++ycls)
        for (int xcls = 0; xcls < 3; ++xcls)
            for (int own = 0; own < 2; ++own)
                for (int cw = 0; cw < 3; ++cw)
                    for (int ce = 0; ce < 3; ++ce)
                        for (int cs = 0; cs < 3; ++cs)
                            for (int cn = 0; cn < 3; ++cn) {
                                const FvmRow r = fvm_row(Do[own], Dn[cw], Dn[ce], Dn[cs], Dn[cn], xcls, ycls, dx, dy, CL, CR);
                                double *row = rows + (size_t)native3_row(ycls, xcls, own, cw, ce, cs, cn) * 6;
                                row[0] = r.a0; row[1] = r.aW; row[2] = r.aE; row[3] = r.aS; row[4] = r.aN; row[5] = r.b;
                            }
}

}  // namespace deff
