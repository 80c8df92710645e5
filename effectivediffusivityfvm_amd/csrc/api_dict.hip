// api_dict.hip -- the row dictionary of an explicit system (kernels_dict.hpp): what turns a host-assembled or imported
// system with few distinct rows into the matrix-free form (codes + tables) the fast kernels run on.  See ctx.hpp for the
// file map.
#include "ctx.hpp"
#include "kernels_dict.hpp"

// Harvest the row dictionary of the explicit system (kernels_dict.hpp).  On success the context
// also has a matrix-free form (codes + tables); when the system has too many distinct rows it
// simply keeps running on the explicit kernels.
static int try_dict(deff_ctx *c)
{
    c->dict_tried = true;
    c->dict_outcome = 0; c->dict_rows = 0;
    if (!c->have_explicit) return DEFF_OK;
    const size_t S = DICT_SLOTS;
    const size_t bytes = S * (8 + 4 + 8) + 16 + S * 2 + (size_t)LUT_MAX_ROWS * (8 + 48);
    TRY(ensure_scratch(c, bytes));
    char *base = (char *)c->scratch;
    DictTable t;
    t.key = (unsigned long long *)base;
    t.rep = (unsigned long long *)(base + S * 8);
    t.count = (unsigned int *)(base + S * 16);
    t.flags = (unsigned int *)(base + S * 20);
    uint16_t *d_slot2code = (uint16_t *)(base + S * 20 + 16);
    unsigned long long *d_cells = (unsigned long long *)(base + S * 22 + 16);
    double *d_rows = (double *)(base + S * 22 + 16 + (size_t)LUT_MAX_ROWS * 8);
    HIP_TRY(hipMemsetAsync(base, 0, S * 20 + 16, c->stream));
    const CoefSoA planes = soa_of(c);
    hipLaunchKernelGGL(k_dict_insert, dim3(grid_for(c->n, 4096)), dim3(256), 0, c->stream, planes, c->n, t);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> key(S), rp(S);
    std::vector<unsigned int> cnt(S);
    unsigned int flags[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(key.data(), t.key, S * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(rp.data(), t.rep, S * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(cnt.data(), t.count, S * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(flags, t.flags, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[0]) { c->dict_outcome = 3; return DEFF_OK; }        // table overflow: far too many rows
    struct Ent { unsigned int count; unsigned slot; unsigned long long bits[6]; };
    std::vector<Ent> ents;
    std::vector<unsigned long long> cells;
    for (unsigned sl = 0; sl < S; ++sl)
        if (key[sl]) {
            if ((int)ents.size() + 2 > LUT_MAX_ROWS) { c->dict_outcome = 2; return DEFF_OK; }   // no seat left beside the zero row
            ents.push_back(Ent{cnt[sl], sl, {0, 0, 0, 0, 0, 0}});
            cells.push_back(rp[sl] - 1);
        }
    if (ents.empty()) return DEFF_OK;
    // one representative row per slot, in slot order: the code order below is decided by the rows themselves, so which
    // cell of a slot arrived first (it differs from run to run) never shows in a code
    const int nrows = (int)ents.size();
    HIP_TRY(hipMemcpyAsync(d_cells, cells.data(), cells.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dict_gather, dim3((nrows + 255) / 256), dim3(256), 0, c->stream, planes, d_cells, nrows, d_rows);
    HIP_TRY(hipGetLastError());
    std::vector<double> slot_rows((size_t)nrows * 6);
    HIP_TRY(hipMemcpyAsync(slot_rows.data(), d_rows, slot_rows.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < nrows; ++k) memcpy(ents[k].bits, &slot_rows[(size_t)k * 6], 48);
    // most populous rows first: the 32 commonest rows then share one conflict-free LDS bank row.  Ties: the six doubles' bit
    // patterns as unsigned integers, in plane order -- the numbering is a function of the system alone
    std::sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) {
        if (a.count != b.count) return a.count > b.count;
        return std::lexicographical_compare(a.bits, a.bits + 6, b.bits, b.bits + 6);
    });
    std::vector<uint16_t> slot2code(S, 0xFFFFu);
    std::vector<double> rows((size_t)nrows * 6);
    for (int k = 0; k < nrows; ++k) {
        slot2code[ents[k].slot] = (uint16_t)((k + 1) * 8);
        memcpy(&rows[(size_t)k * 6], ents[k].bits, 48);
    }
    HIP_TRY(hipMemcpyAsync(d_slot2code, slot2code.data(), S * 2, hipMemcpyHostToDevice, c->stream));
    TRY(dev_alloc(&c->code, c->n));
    c->codes3_valid = false;
    hipLaunchKernelGGL(k_dict_encode, dim3(grid_for(c->n, 4096)), dim3(256), 0, c->stream, planes, c->n, c->nx, c->nxt, t,
                       d_slot2code, c->code);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flags, t.flags, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flags[1]) { c->dict_outcome = 4; return DEFF_OK; }        // hash collision (astronomically unlikely): stay explicit
    c->lut_nrows = nrows + 1;
    c->lut_rows.assign((size_t)c->lut_nrows * 6, 0.0);
    memcpy(&c->lut_rows[6], rows.data(), rows.size() * 8);
    c->lut_allb = flags[2] != 0;
    c->lut_omega = NAN;
    c->have_matfree = true;
    c->links_sym = 0;
    c->dict_outcome = 1; c->dict_rows = nrows;
    return DEFF_OK;
}

// The dictionary of an explicit system for a solver that runs on the matrix-free form only (deff_solve_cg): harvested under
// plan_sweeps' conditions, whatever kernel the sweeps are set to.
int ensure_dictionary(deff_ctx *c)
{
    if (!c->have_matfree && c->have_explicit && !c->dict_tried && c->dict_enabled && !c->wrap_links) TRY(try_dict(c));
    return DEFF_OK;
}

// The matrix-free form as the kernels see it: the table's rows (row 0 = the zero row) and every cell's code, pad column included.
extern "C" int deff_get_dictionary(deff_ctx *c, double *rows, uint16_t *codes)
try {
    if (!c) return fail(DEFF_EINVAL, "ctx is NULL");
    if (!c->have_matfree) return fail(DEFF_ESTATE, "no matrix-free form: the system has no row dictionary");
    if (!rows && !codes) return fail(DEFF_EINVAL, "NULL argument");
    if (rows) memcpy(rows, c->lut_rows.data(), sizeof(double) * 6 * (size_t)c->lut_nrows);
    if (codes) {
        TRY(use_device(c));
        HIP_TRY(hipMemcpyAsync(codes, c->code, sizeof(uint16_t) * c->n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return DEFF_OK;
}
DEFF_API_CATCH
