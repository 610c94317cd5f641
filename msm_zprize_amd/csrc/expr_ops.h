// Gate expressions over resident scalar sets, as one stage: sums of products of rotated columns (msmz_scalars_expr).
// ExprOps owns no device buffer -- the program travels as a kernel argument and the one word that comes back is the
// meta block's -- and reaches the engine through the SetsCore it is built with (sets_core.h).  ResidentSets (resident.h)
// forwards the IEngine method here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/msmz.h"
#include "expr_kernels.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class ExprOps {
  using Core = SetsCore<Cfg>;
  using Fr = typename Cfg::Fr;

 public:
  explicit ExprOps(Core& core) : core_(core) {}

  // msmz_scalars_expr: the compile step (expr_kernels.h), the handles and the overlap rule, the coefficients, then ONE
  // launch, of the register-resident kernel for a program of few operands and of the general one otherwise (the same
  // bytes either way); the error word (a resident record >= q in a column some factor names) comes back behind the ONE host wait.
  int scalars_expr(const msmz_expr& e, uint64_t first_out, uint64_t* out_handle) {
    if (!out_handle) return MSMZ_ERR_ARG;
    ExprProgram P;
    uint8_t named[EXPR_MAX_COLUMNS];
    if (int st = expr_compile(e, &P, named)) return st;
    if (*out_handle == 0 && first_out != 0) return MSMZ_ERR_ARG;
    const uint32_t* base[EXPR_MAX_COLUMNS];
    for (uint32_t c = 0; c < e.n_columns; c++) {
      const msmz_expr_column& col = e.columns[c];
      if (!(base[c] = core_.handles_.range(col.handle, 1, col.first, e.n, 8))) return MSMZ_ERR_ARG;
      if (col.handle == *out_handle && !expr_overlap_ok(named[c], col.first, first_out, e.n)) return MSMZ_ERR_ARG;
    }
    uint32_t* out = nullptr;
    if (*out_handle && !(out = core_.handles_.range(*out_handle, 1, first_out, e.n, 8))) return MSMZ_ERR_ARG;
    for (uint32_t o = 0; o < P.n_ops; o++) P.op[o].base = base[P.op[o].column];
    if (int st = expr_coeffs<Fr>(e, &P)) return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    Handle hd;
    if (int st = core_.fresh_out(e.n, &hd, &out)) return st;
    const dim3 grid((uint32_t)((e.n + EXPR_THREADS - 1) / EXPR_THREADS)), block(EXPR_THREADS);
    const int st = core_.checked([&](uint32_t* d_err) {   // a resident record >= group order
      if (P.n_ops <= (uint32_t)EXPR_REGISTER_SLOTS)
        hipLaunchKernelGGL((k_scalars_expr_slots<Fr, EXPR_REGISTER_SLOTS>), grid, block, 0, core_.stream_, out, P, d_err);
      else
        hipLaunchKernelGGL((k_scalars_expr<Fr>), grid, block, 0, core_.stream_, out, P, d_err);
    });
    return st || !hd.mem.p ? st : core_.add_handle(std::move(hd), out_handle);
  }

 private:
  Core& core_;
};

}  // namespace msmz
