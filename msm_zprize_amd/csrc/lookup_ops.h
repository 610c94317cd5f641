// Lookup arguments over resident scalar sets, as one stage: the multiplicities of a column in a table.  LookupOps owns
// the hash index, the counts and the result record, and reaches the engine through the SetsCore it is built with
// (sets_core.h).  ResidentSets (resident.h) forwards the IEngine method here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/msmz.h"
#include "lookup_kernels.h"
#include "sets_core.h"

namespace msmz {

template <class Cfg>
class LookupOps {
  using Core = SetsCore<Cfg>;
  using Fr = typename Cfg::Fr;

 public:
  explicit LookupOps(Core& core) : core_(core) {}

  // f(buffer) for every device buffer of the stage: all scratch, undefined at the start of every call
  template <class Fn>
  void each_scratch(Fn f) {
    f(lookup_slots_), f(lookup_count_), f(lookup_res_);
  }

  // msmz_scalars_lookup: the index and the counts are cleared (scratch is undefined at the start of a call), then
  // k_lookup_insert, k_lookup_count (k_lookup_count_small for a table of at most LK_SMALL_TABLE entries) and
  // k_lookup_emit; the error word, the three result words and, if asked for, the positions behind them come back in ONE
  // copy behind the ONE host wait.  Both inputs are gathered, so the destination may meet neither range at all.
  int scalars_lookup(const msmz_lookup& l, uint64_t first_out, uint64_t* out_handle, msmz_lookup_result* res) {
    if (!out_handle || l.flags || l.table_n == 0 || l.col_n == 0 || l.table_n > LK_MAX_TABLE || l.col_n >> 32) return MSMZ_ERR_ARG;
    const uint64_t tn = l.table_n, cn = l.col_n;
    if (*out_handle && ((*out_handle == l.table_handle && ranges_meet(l.table_first, tn, first_out, tn)) ||
                        (*out_handle == l.col_handle && ranges_meet(l.col_first, cn, first_out, tn))))
      return MSMZ_ERR_ARG;
    const uint32_t* T = nullptr;
    const uint32_t* Fc = nullptr;
    uint32_t* out = nullptr;
    if (int st = core_.resolve({{l.table_handle, l.table_first, &T, tn}, {l.col_handle, l.col_first, &Fc, cn}}, tn, first_out,
                               *out_handle, &out))
      return st;
    MSMZ_HIP(hipSetDevice(core_.device_));
    hipStream_t stream = core_.stream_;
    const uint32_t slots = lk_slots(tn);
    if (int st = lookup_slots_.ensure((size_t)slots * 4)) return st;
    if (int st = lookup_count_.ensure(tn * 4)) return st;
    Handle hd;
    if (int st = core_.fresh_out(tn, &hd, &out)) return st;
    typename Core::Record rec;   // word LK_RES_ERR: the error word; first_missing starts as "none"; then the positions
    rec.head = (size_t)LK_RES_WORDS * 4, rec.err_word = LK_RES_ERR, rec.preset_word = LK_RES_FIRST;
    rec.tail = l.positions ? cn * 4 : 0;
    const int st = core_.recorded(lookup_res_, rec.head + rec.tail, [&](uint32_t* d_res) {
      uint32_t* d_pos = l.positions ? d_res + LK_RES_WORDS : nullptr;
      uint32_t* d_slots = lookup_slots_.as<uint32_t>();
      uint32_t* d_count = lookup_count_.as<uint32_t>();
      if (hipMemsetAsync(d_slots, 0xff, (size_t)slots * 4, stream) != hipSuccess ||
          hipMemsetAsync(d_count, 0, tn * 4, stream) != hipSuccess)
        return;   // (recorded reports it)
      const dim3 block(LK_THREADS), tgrid((uint32_t)((tn + LK_THREADS - 1) / LK_THREADS)),
          cgrid((uint32_t)((cn + LK_THREADS - 1) / LK_THREADS));
      hipLaunchKernelGGL((k_lookup_insert<Fr>), tgrid, block, 0, stream, d_slots, slots - 1, T, (uint32_t)tn, d_res);
      if (tn <= LK_SMALL_TABLE)
        hipLaunchKernelGGL((k_lookup_count_small<Fr>), dim3(lk_small_groups(cn)), block, 0, stream, d_count, d_res, d_pos,
                           d_slots, slots - 1, T, (uint32_t)tn, Fc, (uint32_t)cn);
      else
        hipLaunchKernelGGL((k_lookup_count<Fr>), cgrid, block, 0, stream, d_count, d_res, d_pos, d_slots, slots - 1, T, Fc,
                           (uint32_t)cn);
      hipLaunchKernelGGL((k_lookup_emit<Fr>), tgrid, block, 0, stream, out, (const uint32_t*)d_count, (uint32_t)tn);
    }, rec);
    if (st) return st;   // (hd frees a fresh destination)
    const uint32_t* w = core_.h_res_.template as<const uint32_t>();
    if (l.positions) memcpy(l.positions, w + LK_RES_WORDS, cn * 4);
    if (res) {
      res->n_missing = w[LK_RES_MISSING];
      res->first_missing = w[LK_RES_FIRST] == LK_EMPTY ? UINT64_MAX : w[LK_RES_FIRST];
      res->n_distinct = w[LK_RES_DISTINCT];
    }
    return hd.mem.p ? core_.add_handle(std::move(hd), out_handle) : (int)MSMZ_OK;
  }

 private:
  Core& core_;
  DevBuf lookup_slots_;   // the hash index, one table index or LK_EMPTY per slot
  DevBuf lookup_count_;   // one count per table entry
  DevBuf lookup_res_;     // the error word and the three result words, then one position per column entry
};

}  // namespace msmz
