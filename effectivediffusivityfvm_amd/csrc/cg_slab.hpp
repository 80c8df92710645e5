// cg_slab.hpp -- conjugate gradients over row slabs, the seam between the two files that build it: api_cg.hip holds every CG
// kernel (kernels_cg_slab.hpp among them) and enqueues the steps of ONE slab below on that slab's stream; api_slab.hip holds
// the loop over the slabs and what travels between them (slab_solve_cg).  No step waits on the host except slcg_read.
#pragma once
#include "ctx.hpp"

constexpr int CG_SLAB_SLOT = 3;               // doubles per slab and gather (kernels_cg_slab.hpp: SLCG_SLOT)
constexpr int CG_SLAB_PHASES = 3;             // gathers in flight use buffers of their own: A (p.Ap), B (r.z, r.r), C (check / verdict)
constexpr int CG_MAX_RESTARTS = 8;            // true-residual rounds that may send a finished solve back into the iteration

struct CgSlab {
    deff_ctx *c = nullptr;
    int nslabs = 1, me = 0;                   // slabs of the image, this one's index
    double *all = nullptr;                    // device [CG_SLAB_PHASES][nslabs][CG_SLAB_SLOT], slot `me` written by this slab's kernels
    // by slcg_setup
    int ntx = 0, kr = 0, m_lo = 0, m_hi = 0;
    unsigned items = 0;
    double tol2 = 0;
    long long max_iter = 0;
    int64_t k = 0;                            // iterations enqueued (parity of the p buffers)
    std::string refusal;                      // why this slab cannot run CG ("" = it can) ...
    int status = 0;                           // ... and the status that goes with it (DEFF_EINVAL, DEFF_ESTATE, DEFF_ENOMEM)
};

struct CgSlabState {
    long long iters;
    double rel;
    int done;
    unsigned restarted;                       // the last mode-1 check sent the solve back
};

static inline double *slcg_slot(const CgSlab &s, int phase, int q)
{
    return s.all + ((size_t)phase * s.nslabs + q) * CG_SLAB_SLOT;
}

// Checks, table, buffers, admissibility of the slab's window; the verdict (0 = admissible, 1 = not symmetric, else 1 - the
// status of the host's own checks) lands in slot C of this slab and is gathered like a sum, so that every slab refuses or
// none.  A refusal of this slab (a failed allocation among them) is DEFF_OK here with s->refusal and s->status set; only a
// failed HIP call returns at once.  What deff_get_plan reports changes with slcg_commit, once every slab is admitted.
int slcg_setup(CgSlab *s, double rtol, int64_t max_iter);
void slcg_commit(CgSlab *s);
int slcg_dir(CgSlab *s);                       // p' and the partials of p'.Ap'; this slab's sum -> slot A
int slcg_alpha_update(CgSlab *s);              // (slot A gathered) alpha; x, r; this slab's sums -> slot B
int slcg_beta(CgSlab *s);                      // (slot B gathered, r's halo rows exchanged) stop or beta
int slcg_resid(CgSlab *s);                     // (x's halo rows exchanged) r = b - A x; this slab's sums -> slot C
int slcg_check(CgSlab *s, int mode, int allow_restart);   // (slot C gathered, r's halo rows exchanged)
int slcg_read(CgSlab *s, CgSlabState *out);    // the slab's scalars -> host; waits for the slab's stream
