// Stage-level test hooks (include/msmz_test.h): each runs ONE device routine of the MSM pipeline, or one phase of an
// engine, on caller-supplied inputs and returns its raw output.  They never take part in an MSM and write to no member
// of the engine they are given besides its device buffers.
#pragma once
#include "../../include/msmz_test.h"
#include "engine.h"
#include "test_kernels.h"

namespace msmz {

// The twelve msmz_test_* stage entry points of an engine whatever its curve; arguments as in msmz_test.h and TestHooks.
class ITestHooks {
 public:
  virtual ~ITestHooks() {}
  virtual int test_field(int, const uint8_t*, const uint8_t*, uint64_t, uint8_t*) = 0;
  virtual int test_field_limbs(int, const int32_t*, const int32_t*, uint64_t, int32_t*, uint8_t*) = 0;
  virtual int test_field_rows(int, const int32_t*, const int32_t*, uint64_t, uint32_t, int32_t*, uint8_t*) = 0;
  virtual int test_glv(const uint8_t*, uint64_t, uint8_t*, uint8_t*, uint8_t*) = 0;
  virtual int test_digits(const uint8_t*, uint64_t, int, int, int, uint32_t*) = 0;
  virtual int test_sort(const uint8_t*, uint64_t, int, int, int, uint32_t*, uint32_t*, uint64_t, uint32_t*, uint64_t) = 0;
  virtual int test_sort_ex(const msmz_test_sort_args&) = 0;
  virtual int test_point(int, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint64_t, uint8_t*) = 0;
  virtual int test_point_raw(int, const uint8_t*, const uint8_t*, const uint8_t*, uint64_t, int, uint8_t*) = 0;
  virtual int test_batch_add(int, int, const uint8_t*, const uint8_t*, uint64_t, const uint8_t*, const uint8_t*, uint64_t,
                             const uint32_t*, uint64_t, uint64_t, uint8_t*, uint32_t*) = 0;
  virtual int test_reduce(const msmz_test_reduce_args&) = 0;
  virtual int test_plan(const msmz_test_plan_args&) = 0;
};

// The regions of an engine's staging buffer that one hook call copies its host arrays into and its results out of, each
// at 256-byte alignment.  in() / out() lay them out and return their ids; an optional array the caller left out (null)
// gets none: id -1, device pointer null.  upload() selects the device, sizes the buffer and queues the copies in; after
// the hook's launches, download() queues the copies out and waits for them.
struct Staging {
  struct Region {
    const void* src;   // the host array copied in, or
    void* dst;         // the host array copied out
    size_t off, bytes;
  };
  int device;
  hipStream_t stream;
  DevBuf& buf;
  std::vector<Region> regions;
  size_t total = 0;

  int in(const void* host, size_t bytes) { return add({host, nullptr, total, bytes}, host); }
  int out(void* host, size_t bytes) { return add({nullptr, host, total, bytes}, host); }
  int add(const Region& r, const void* host) {
    if (!host) return -1;
    regions.push_back(r);
    total += (r.bytes + 255) & ~(size_t)255;
    return (int)regions.size() - 1;
  }
  template <class T>
  T* at(int id) const {
    return id < 0 ? nullptr : reinterpret_cast<T*>(buf.as<uint8_t>() + regions[id].off);
  }
  int upload() {
    MSMZ_HIP(hipSetDevice(device));
    if (int st = buf.ensure(total)) return st;
    for (const Region& r : regions)
      if (r.src && r.bytes)
        MSMZ_HIP(hipMemcpyAsync(buf.as<uint8_t>() + r.off, r.src, r.bytes, hipMemcpyHostToDevice, stream));
    return MSMZ_OK;
  }
  int download() {
    MSMZ_HIP(hipGetLastError());
    for (const Region& r : regions)
      if (r.dst && r.bytes)
        MSMZ_HIP(hipMemcpyAsync(r.dst, buf.as<uint8_t>() + r.off, r.bytes, hipMemcpyDeviceToHost, stream));
    MSMZ_HIP(hipStreamSynchronize(stream));
    return MSMZ_OK;
  }
};

// The hooks of one engine.  A friend of Engine<Cfg>: the hooks launch on its stream, stage through stage_ and meta_, fill
// the buffers its stages share (slots_, bfin_, rscan_, desc_) as inputs, and run its own sort stage (BucketSort::run,
// sort.h), reduction stage (the public interface of BucketReduce, reduce.h), batch adder (batch_adder, batch_add.h) and
// plan_phase.  Its planner and its reduction thresholds they only read, and vary in copies.
template <class Cfg>
class TestHooks : public ITestHooks {
  using E = Engine<Cfg>;
  using F = typename Cfg::F;
  using Fr = typename Cfg::Fr;
  static constexpr bool TE = Cfg::TE;
  using P = typename Cfg::P;

 public:
  explicit TestHooks(E& engine) : eng_(engine) {}

  int test_field(int op, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out) override {
    if (!a || !b || !out || n == 0 || n > (1u << 22)) return MSMZ_ERR_ARG;
    const size_t eb = (size_t)E::FE_BYTES * n;
    Staging sg = staging();
    const int ia = sg.in(a, eb), ib = sg.in(b, eb), io = sg.out(out, eb);
    int st;
    if ((st = sg.upload()) || (st = eng_.slots_.ensure(((size_t)n + 64) * SlotFmt<F>::WORDS * 4))) return st;
    hipLaunchKernelGGL((k_test_field<F>), dim3((n + 63) / 64), dim3(64), 0, eng_.stream_, sg.at<uint32_t>(io),
                       sg.at<const uint32_t>(ia), sg.at<const uint32_t>(ib), (uint32_t)n, op,
                       eng_.slots_.template as<uint32_t>());
    return sg.download();
  }

  int test_field_limbs(int op, const int32_t* a, const int32_t* b, uint64_t n, int32_t* raw, uint8_t* canon) override {
    if (!a || !b || !raw || !canon || n == 0 || n > (1u << 22) || op < 0 || op >= TFL_COUNT) return MSMZ_ERR_ARG;
    const size_t lb = (size_t)4 * F::N * n, eb = (size_t)E::FE_BYTES * n;
    Staging sg = staging();
    const int ia = sg.in(a, lb), ib = sg.in(b, lb), iraw = sg.out(raw, lb), icanon = sg.out(canon, eb);
    int st;
    if ((st = sg.upload()) || (st = eng_.slots_.ensure(((size_t)n + 64) * SlotFmt<F>::WORDS * 4))) return st;
    hipLaunchKernelGGL((k_test_field_limbs<F>), dim3((n + 63) / 64), dim3(64), 0, eng_.stream_, sg.at<int32_t>(iraw),
                       sg.at<uint32_t>(icanon), sg.at<const int32_t>(ia), sg.at<const int32_t>(ib), (uint32_t)n, op,
                       eng_.slots_.template as<uint32_t>());
    return sg.download();
  }

  int test_field_rows(int op, const int32_t* a, const int32_t* b, uint64_t n, uint32_t live_rows, int32_t* raw,
                      uint8_t* canon) override {
    if (!a || !b || !raw || !canon || n == 0 || n > (1u << 22) || op < 0 || op >= TFR_COUNT || live_rows == 0 ||
        live_rows > 15)
      return MSMZ_ERR_ARG;
    const size_t lb = (size_t)4 * F::N * n, eb = (size_t)E::FE_BYTES * n;
    Staging sg = staging();
    const int ia = sg.in(a, lb), ib = sg.in(b, lb), iraw = sg.out(raw, lb), icanon = sg.out(canon, eb);
    if (int st = sg.upload()) return st;
    const uint32_t per_wave = (uint32_t)__builtin_popcount(live_rows);
    hipLaunchKernelGGL((k_test_field_rows<F>), dim3((uint32_t)((n + per_wave - 1) / per_wave)), dim3(64), 0, eng_.stream_,
                       sg.at<int32_t>(iraw), sg.at<uint32_t>(icanon), sg.at<const int32_t>(ia), sg.at<const int32_t>(ib),
                       (uint32_t)n, op, live_rows);
    return sg.download();
  }

  int test_glv(const uint8_t* s, uint64_t n, uint8_t* s0, uint8_t* s1, uint8_t* neg) override {
    if (!Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    if (!s || !s0 || !s1 || !neg || n == 0 || n > (1u << 22)) return MSMZ_ERR_ARG;
    Staging sg = staging();
    const int is = sg.in(s, 32 * n), i0 = sg.out(s0, 16 * n), i1 = sg.out(s1, 16 * n), ineg = sg.out(neg, 2 * n);
    if (int st = sg.upload()) return st;
    hipLaunchKernelGGL((k_test_glv<Fr>), dim3((n + 255) / 256), dim3(256), 0, eng_.stream_, sg.at<uint32_t>(i0),
                       sg.at<uint32_t>(i1), sg.at<uint8_t>(ineg), sg.at<const uint32_t>(is), (uint32_t)n);
    return sg.download();
  }

  int test_digits(const uint8_t* s, uint64_t n, int c, int K, int glv, uint32_t* digits) override {
    if (!s || !digits || n == 0 || n > (1u << 22) || c < 2 || c > 24 || K < 1 || K > kMaxWindows) return MSMZ_ERR_ARG;
    if (glv && !Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    Staging sg = staging();
    const int is = sg.in(s, 32 * n), id = sg.out(digits, (size_t)(glv ? 2 : 1) * n * K * 4);
    if (int st = sg.upload()) return st;
    if (glv) {
      if constexpr (Fr::HAS_GLV)
        hipLaunchKernelGGL((k_test_digits<Fr, true>), dim3((n + 255) / 256), dim3(256), 0, eng_.stream_,
                           sg.at<uint32_t>(id), sg.at<const uint32_t>(is), (uint32_t)n, c, K);
    } else {
      hipLaunchKernelGGL((k_test_digits<Fr, false>), dim3((n + 255) / 256), dim3(256), 0, eng_.stream_,
                         sg.at<uint32_t>(id), sg.at<const uint32_t>(is), (uint32_t)n, c, K);
    }
    return sg.download();
  }

  // msmz_test_sort: test_sort_ex with one problem, one window per bucket set, no bound, no fold, pts_n = n; a flagged
  // scalar is MSMZ_ERR_RANGE here, and refs need room for the entries there are only
  int test_sort(const uint8_t* s, uint64_t n, int c, int glv, int force_fallback, uint32_t* geom, uint32_t* off,
                uint64_t off_cap, uint32_t* refs, uint64_t refs_cap) override {
    if (!geom) return MSMZ_ERR_ARG;
    uint32_t gw[MSMZ_TS_GEOM_WORDS], meta[3];
    msmz_test_sort_args a;
    memset(&a, 0, sizeof(a));
    a.scalars_le32 = s;
    a.n = a.pts_n = n;
    a.nprob = a.factor = 1;
    a.c = c;
    a.glv = glv;
    a.force_fallback = force_fallback;
    a.geom = gw;
    a.geom_cap = MSMZ_TS_GEOM_WORDS;
    a.meta = meta;
    if (int st = test_sort_ex(a)) return st;
    if (meta[0] & 4u) return MSMZ_ERR_RANGE;
    const uint32_t nb = gw[MSMZ_TS_NB], n_entries = meta[1];
    const uint32_t g8[8] = {gw[MSMZ_TS_C], gw[MSMZ_TS_K], gw[MSMZ_TS_KEFF], gw[MSMZ_TS_L], nb, n_entries, meta[2],
                            gw[MSMZ_TS_SPREAD]};
    memcpy(geom, g8, sizeof(g8));
    if (off) {
      if (off_cap < (uint64_t)nb + 1) return MSMZ_ERR_ARG;
      MSMZ_HIP(hipMemcpy(off, eng_.sort_.off(), ((size_t)nb + 1) * 4, hipMemcpyDeviceToHost));
    }
    if (refs) {
      if (refs_cap < n_entries) return MSMZ_ERR_ARG;
      if (n_entries) MSMZ_HIP(hipMemcpy(refs, eng_.sort_.refs(), (size_t)n_entries * 4, hipMemcpyDeviceToHost));
    }
    return MSMZ_OK;
  }

  // The bucket sort at any geometry an MSM plans (msmz_test.h): the planner's plan and layout for the caller's options,
  // then the engine's sort stage (BucketSort::run, sort.h).  Everything the kernels index with comes from that plan; what the caller controls
  // beyond it (capacities, pts_n, copy_stride) is checked here before anything is launched.
  int test_sort_ex(const msmz_test_sort_args& a) override {
    const uint64_t n = a.n, pts_n = a.pts_n ? a.pts_n : a.n;
    if (!a.scalars_le32 || n == 0 || n > (1u << 22) || a.nprob < 1 || a.nprob > 64) return MSMZ_ERR_ARG;
    if (a.c < 0 || a.c > 24 || a.scalar_bits < 0 || a.scalar_bits > 256 || a.factor > (uint32_t)kMaxWindows) return MSMZ_ERR_ARG;
    if (pts_n < n || pts_n > (1u << 30)) return MSMZ_ERR_ARG;
    if (a.glv && !Fr::HAS_GLV) return MSMZ_ERR_UNSUPPORTED;
    if (a.geom && a.geom_cap < MSMZ_TS_GEOM_WORDS) return MSMZ_ERR_ARG;
    msmz_opts opt;
    memset(&opt, 0, sizeof(opt));
    opt.c = a.c;
    opt.reserved[1] = a.scalar_bits;
    Planner<Fr> pr = eng_.planner_;
    pr.k.force_atomic_sort = pr.k.force_atomic_sort || a.force_fallback != 0;
    Plan pl;
    int st = pr.make_plan(pl, n, a.glv != 0, opt, (uint32_t)pts_n, !TE, 0, a.allow_fold != 0, a.nprob,
                          a.factor > 1 ? a.factor : 1);
    if (st) return st;
    const SortLayout sl = pr.sort_layout(pl);
    const SortGeom& g = sl.geom;
    const uint64_t cap_entries = (uint64_t)pl.nprob * pl.K * pl.M;
    if (pl.K > kMaxWindows || cap_entries > kMaxBatchEntries) return MSMZ_ERR_ARG;
    if (!sl.two_level && (pl.nprob > 1 || pl.F > 1)) return MSMZ_ERR_UNSUPPORTED;
    // the largest reference: the last entry (of the second half: moved up by endo_delta), in the last copy
    const uint32_t W = Planner<Fr>::set_windows(pl);
    if ((uint64_t)pl.M - 1 + pl.endo_delta + (uint64_t)(W - 1) * a.copy_stride >= (1ull << 31)) return MSMZ_ERR_ARG;
    const uint32_t per_tile = pl.glv ? COARSE_TILE / 2 : COARSE_TILE;
    const size_t n_off = (size_t)pl.nprob * pl.nb + 1, n_bins = (size_t)pl.nprob * g.sbins + 1;
    if (a.geom) {
      const uint32_t gw[MSMZ_TS_GEOM_WORDS] = {
          (uint32_t)pl.c, (uint32_t)pl.K, (uint32_t)pl.Keff, pl.L, pl.nb, (uint32_t)g.fb, (uint32_t)g.fbt, g.ncb, g.ncbt,
          sl.nbins, g.sbins, sl.fbins, sl.fine_top, (uint32_t)pl.spread, (uint32_t)pl.fold_shift, (uint32_t)pl.fold_rows,
          W, (uint32_t)g.mbits, (uint32_t)g.idx_bits, (uint32_t)sl.cspec, sl.two_level ? 1u : 0u,
          sl.two_level ? (pl.n + per_tile - 1) / per_tile : 0u, (uint32_t)(pl.sbits ? pl.sbits : 256), pl.endo_delta};
      memcpy(a.geom, gw, sizeof(gw));
    }
    if (!a.meta && !a.off && !a.refs && !a.bins && !a.packed) return MSMZ_OK;   // the geometry only
    if ((a.off && a.off_cap < n_off) || (a.refs && a.refs_cap < cap_entries)) return MSMZ_ERR_ARG;
    if (sl.two_level && ((a.bins && a.bins_cap < n_bins) || (a.packed && a.packed_cap < cap_entries))) return MSMZ_ERR_ARG;

    Staging sg = staging();
    const int is = sg.in(a.scalars_le32, (size_t)32 * pl.nprob * n);
    if ((st = sg.upload())) return st;
    Run run = eng_.new_run(opt);
    if ((st = eng_.sort_.run(pl, sl, sg.at<const uint32_t>(is), run, eng_.stream_, eng_.meta_.template as<MsmMeta>(),
                             a.copy_stride)) ||
        (st = eng_.fetch_meta(run)))
      return st;
    const uint32_t n_entries = run.n_entries;
    if (n_entries > cap_entries) return MSMZ_ERR_HIP;   // (a broken count: nothing is copied by it)
    if (a.meta) {
      a.meta[0] = eng_.h_meta_->error;
      a.meta[1] = n_entries;
      a.meta[2] = run.max_bucket;
    }
    if (a.off) MSMZ_HIP(hipMemcpy(a.off, eng_.sort_.off(), n_off * 4, hipMemcpyDeviceToHost));
    if (a.refs && n_entries) MSMZ_HIP(hipMemcpy(a.refs, eng_.sort_.refs(), (size_t)n_entries * 4, hipMemcpyDeviceToHost));
    if (sl.two_level) {
      if (a.bins) MSMZ_HIP(hipMemcpy(a.bins, eng_.sort_.bins(), n_bins * 4, hipMemcpyDeviceToHost));
      if (a.packed && n_entries)
        MSMZ_HIP(hipMemcpy(a.packed, eng_.sort_.packed(), (size_t)n_entries * 4, hipMemcpyDeviceToHost));
    }
    return MSMZ_OK;
  }

  int test_point(int op, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b, const uint8_t* b_inf, uint64_t n,
                 uint8_t* out) override {
    if (!a || !b || !out || n == 0 || n > (1u << 20)) return MSMZ_ERR_ARG;
    const size_t pb = (size_t)2 * E::FE_BYTES * n;
    Staging sg = staging();
    const int ia = sg.in(a, pb), ib = sg.in(b, pb), iai = sg.in(a_inf, n), ibi = sg.in(b_inf, n), io = sg.out(out, pb);
    if (int st = sg.upload()) return st;
    const uint64_t threads = (op == TP_ADD_X4 || op == TP_DBL_X4) ? 4 * n : n;
    hipLaunchKernelGGL((k_test_point<P>), dim3((threads + 63) / 64), dim3(64), 0, eng_.stream_, sg.at<uint32_t>(io),
                       sg.at<const uint32_t>(ia), sg.at<const uint32_t>(ib), sg.at<const uint8_t>(iai),
                       sg.at<const uint8_t>(ibi), (uint32_t)n, op);
    return sg.download();
  }

  int test_point_raw(int op, const uint8_t* a, const uint8_t* b, const uint8_t* neg, uint64_t n, int L,
                     uint8_t* out) override {
    if (!a || !b || !out || n == 0 || n > (1u << 20) || op < 0 || op >= TPR_COUNT || L < 0 || L > 4096)
      return MSMZ_ERR_ARG;
    if (TE && op == TPR_MDBL) return MSMZ_ERR_UNSUPPORTED;
    const size_t rb = (size_t)4 * E::FE_BYTES * n, pb = (size_t)2 * E::FE_BYTES * n;
    Staging sg = staging();
    const int ia = sg.in(a, rb), ib = sg.in(b, rb), ineg = sg.in(neg, n), io = sg.out(out, pb);
    if (int st = sg.upload()) return st;
    const bool x4 = op == TPR_ADD_X4 || op == TPR_DBL_X4 || op == TPR_CHAIN_X4;
    const uint64_t threads = op >= TPR_ADD_ROWS ? 64 * n : x4 ? 4 * n : n;   // rows: one wave = one workgroup per element
    hipLaunchKernelGGL((k_test_point_raw<P>), dim3((threads + 63) / 64), dim3(64), 0, eng_.stream_,
                       sg.at<uint32_t>(io), sg.at<const uint32_t>(ia), sg.at<const uint32_t>(ib),
                       sg.at<const uint8_t>(ineg), (uint32_t)n, op, L);
    return sg.download();
  }

  int test_batch_add(int safe, int B, const uint8_t* pxy, const uint8_t* pinf, uint64_t np, const uint8_t* sxy,
                     const uint8_t* sinf, uint64_t ns, const uint32_t* desc, uint64_t n_pairs, uint64_t out_base,
                     uint8_t* out, uint32_t* error) override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;
    constexpr uint64_t CAP = 1u << 22;
    if (!desc || !out || !error || (safe != 0 && safe != 1) || B < 1 || B > MSMZ_BATCH_BMAX) return MSMZ_ERR_ARG;
    if (n_pairs == 0 || n_pairs > CAP || np > CAP || ns > CAP || (np && !pxy) || (ns && !sxy)) return MSMZ_ERR_ARG;
    if (out_base < ns || out_base > CAP) return MSMZ_ERR_ARG;
    // every location names a supplied operand: the kernel reads whatever its descriptors point at
    for (uint64_t k = 0; k < 2 * n_pairs; k++) {
      const uint32_t w = desc[k];
      if ((w & LOC_ORIG) ? (w & 0x3fffffffu) >= np : w >= ns) return MSMZ_ERR_ARG;
    }
    const size_t rec = (size_t)E::RW * 4;
    Staging sg = staging();
    const int ipxy = sg.in(pxy, rec * np), ipinf = sg.in(pinf, np), isxy = sg.in(sxy, rec * ns), isinf = sg.in(sinf, ns);
    const int idesc = sg.in(desc, (size_t)8 * n_pairs), io = sg.out(out, rec * n_pairs);
    int st = sg.upload();
    if (st) return st;
    MsmMeta* d_meta = eng_.meta_.template as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, eng_.stream_));
    DevBuf d_pts;   // the resident point set (freed on every return)
    uint32_t err = 0;
    // slot records 0 .. out_base + n_pairs - 1, as the MSM sizes them
    if ((st = load_operands(d_pts, sg.at<const uint32_t>(ipxy), sg.at<const uint8_t>(ipinf), np,
                            sg.at<const uint32_t>(isxy), sg.at<const uint8_t>(isinf), ns, (uint32_t)(out_base + n_pairs))) ||
        (st = eng_.fetch_error(&err)))
      return st;
    if (err) return MSMZ_ERR_RANGE;   // a coordinate >= p
    eng_.batch_adder().launch((uint32_t)n_pairs, safe != 0, d_pts.as<uint32_t>(), sg.at<const uint2>(idesc),
                              (uint32_t)out_base, d_meta, B);
    MSMZ_HIP(hipGetLastError());
    if constexpr (!TE)
      hipLaunchKernelGGL((k_test_slots_out<F>), dim3((n_pairs + 255) / 256), dim3(256), 0, eng_.stream_,
                         sg.at<uint32_t>(io), eng_.slots_.template as<uint32_t>(), (uint32_t)out_base, (uint32_t)n_pairs);
    if ((st = eng_.fetch_error(error))) return st;
    return sg.download();
  }

  // The bucket reduction on caller-built buckets (msmz_test.h).  The level-selection knobs hold for this call only: they
  // go into copies of the engine's thresholds and planner, and the reduction takes both as arguments.
  int test_reduce(const msmz_test_reduce_args& a) override {
    constexpr int AW = P::ACC_WORDS, NW = F::NW, RW = E::RW;
    constexpr uint64_t CAP = 1u << 20;
    const bool levels = a.mode == MSMZ_TR_LEVELS, locs = a.mode == MSMZ_TR_LOCATIONS;
    if (a.mode < MSMZ_TR_LOCATIONS || a.mode > MSMZ_TR_LEVELS || !a.out_xy) return MSMZ_ERR_ARG;
    if (TE && locs) return MSMZ_ERR_UNSUPPORTED;
    if (a.tail_n > 4096 || a.quad16_max > CAP || a.pairsum_x4_max > CAP || a.rows_max > CAP) return MSMZ_ERR_ARG;
    if (a.n_points > CAP || a.n_slots > CAP || (a.n_points && !a.points_xy) || (a.n_slots && !a.slots_xy)) return MSMZ_ERR_ARG;
    // geometry: a plan of `nsets` bucket sets of window size c, as far as Planner::r2_geom and the hook read one
    Plan pl{};
    pl.nprob = 1;
    pl.F = 1;
    R2Geom g{};   // 2-D modes: the split of the bucket sets, with the caller's NC
    uint32_t nb = 0, n_res = a.nsets;
    if (levels) {
      if (a.nsets < 1 || a.nsets > 64 || a.n_in < 1 || a.n_in > 4096 || a.nc != 0) return MSMZ_ERR_ARG;
      if (a.n_points != (uint64_t)2 * a.nsets * a.n_in) return MSMZ_ERR_ARG;
      pl.Keff = (int)a.nsets;
    } else {
      if (a.c < 2 || a.c > 16 || a.nsets < 1 || a.nsets > 16) return MSMZ_ERR_ARG;
      pl.c = a.c;
      pl.L = 1u << (a.c - 1);
      pl.Keff = pl.K = (int)a.nsets;
      nb = pl.nb = a.nsets * pl.L;
      Planner<Fr> pr = eng_.planner_;
      if (a.nc) pr.k.r2_nc = a.nc;
      g = pr.r2_geom(pl);
      if (a.nc != 0 && ((a.nc & (a.nc - 1)) != 0 || a.nc > g.D)) return MSMZ_ERR_ARG;
      n_res = 2 * a.nsets;
      // every location / chunk range names a supplied operand: the kernels read whatever these point at
      if (locs) {
        if (!a.loc) return MSMZ_ERR_ARG;
        for (uint64_t k = 0; k < (uint64_t)4 * nb; k++) {
          const uint32_t w = a.loc[k];
          if (w == LOC_NONE) {
            k |= 3;   // (the rest of this bucket's words is never read)
            continue;
          }
          if ((w & LOC_ORIG) ? (w & 0x3fffffffu) >= a.n_points : w >= a.n_slots) return MSMZ_ERR_ARG;
        }
      } else {
        if (!a.cscan || a.cscan[nb] > a.n_points) return MSMZ_ERR_ARG;
        for (uint32_t g = 0; g < nb; g++)
          if (a.cscan[g] > a.cscan[g + 1]) return MSMZ_ERR_ARG;
      }
    }
    if (a.scale && locs) return MSMZ_ERR_ARG;
    ReduceKnobs rk = eng_.reduce_knobs_;
    if (a.tail_n) rk.tail_n = a.tail_n;
    if (a.quad16_max) rk.quad16_max = a.quad16_max;
    if (a.pairsum_x4_max) rk.pairsum_x4_max = a.pairsum_x4_max;
    if (a.rows_max) rk.rows_max = a.rows_max;
    const uint32_t n_lines = levels || !a.lines_xy ? 0 : n_res * g.H;

    const size_t np = a.n_points, ns = a.n_slots, rec = (size_t)RW * 4;
    Staging sg = staging();
    const int ipxy = sg.in(a.points_xy, rec * np), ipinf = sg.in(a.points_inf, np);
    const int iscale = sg.in(a.scale, (size_t)E::FE_BYTES * np);
    const int isxy = sg.in(a.slots_xy, rec * ns), isinf = sg.in(a.slots_inf, ns);
    const int ires = sg.out(a.out_xy, rec * n_res), ilines = sg.out(n_lines ? a.lines_xy : nullptr, rec * n_lines);
    int st = sg.upload();
    if (st) return st;
    MsmMeta* d_meta = eng_.meta_.template as<MsmMeta>();
    MSMZ_HIP(hipMemsetAsync(&d_meta->error, 0, 4, eng_.stream_));
    // accumulator records `first .. first + n` of the input points, in the policy's memory format
    auto accs_in = [&](uint32_t* dst, size_t first, size_t n) {
      const uint8_t* d_pinf = sg.at<const uint8_t>(ipinf);
      const uint32_t* d_scale = sg.at<const uint32_t>(iscale);
      if (n)
        hipLaunchKernelGGL((k_test_accs_in<P>), dim3((n + 255) / 256), dim3(256), 0, eng_.stream_, dst,
                           sg.at<const uint32_t>(ipxy) + first * RW, d_pinf ? d_pinf + first : nullptr,
                           d_scale ? d_scale + first * NW : nullptr, (uint32_t)n, &d_meta->error);
    };
    DevBuf d_pts;   // LOCATIONS: the resident point set (freed on every return)
    BucketReduce<Cfg>& red = eng_.reduce_;
    if (levels) {
      const size_t n = (size_t)a.nsets * a.n_in;
      uint32_t *rows, *c;
      if ((st = red.level_inputs(n, &rows, &c))) return st;
      accs_in(rows, 0, n);
      accs_in(c, n, n);
    } else if (locs) {
      if ((st = eng_.bfin_.ensure((size_t)nb * 16))) return st;
      MSMZ_HIP(hipMemcpyAsync(eng_.bfin_.p, a.loc, (size_t)nb * 16, hipMemcpyHostToDevice, eng_.stream_));
      if ((st = load_operands(d_pts, sg.at<const uint32_t>(ipxy), sg.at<const uint8_t>(ipinf), np,
                              sg.at<const uint32_t>(isxy), sg.at<const uint8_t>(isinf), ns, (uint32_t)ns)))
        return st;
    } else {
      if ((st = eng_.slots_.ensure((np + 1) * AW * 4)) || (st = eng_.rscan_.ensure(((size_t)nb + 1) * 4))) return st;
      MSMZ_HIP(hipMemcpyAsync(eng_.rscan_.p, a.cscan, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, eng_.stream_));
      accs_in(eng_.slots_.template as<uint32_t>(), 0, np);
    }
    uint32_t err = 0;
    if ((st = eng_.fetch_error(&err))) return st;
    if (err & 4u) return MSMZ_ERR_RANGE;   // a coordinate or scale >= p
    if (err) return MSMZ_ERR_ARG;          // a zero scale

    if (levels) {
      if ((st = red.levels(rk, a.n_in, a.nsets, eng_.stream_))) return st;
    } else {
      const uint32_t* slots = eng_.slots_.template as<uint32_t>();
      BucketSource src = locs ? BucketSource::locations(slots, d_pts.as<uint32_t>(), eng_.bfin_.template as<uint4>())
                              : BucketSource::chunks(slots, eng_.rscan_.template as<uint32_t>());
      if (a.mode == MSMZ_TR_ACCS_SUMMED && (st = red.bucket_sums(src, nb, eng_.stream_, &src))) return st;
      const uint32_t* lines;   // read out here, before the weighted levels reuse them
      if ((st = red.line_sums(g, rk, src, eng_.stream_, &lines))) return st;
      if (n_lines)
        hipLaunchKernelGGL((k_test_accs_out<P>), dim3((n_lines + 63) / 64), dim3(64), 0, eng_.stream_,
                           sg.at<uint32_t>(ilines), lines, n_lines);
      if ((st = red.weighted_sums(g, rk, eng_.stream_))) return st;
    }
    MSMZ_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_test_accs_out<P>), dim3((n_res + 63) / 64), dim3(64), 0, eng_.stream_, sg.at<uint32_t>(ires),
                       red.final(), n_res);
    return sg.download();
  }

  // The tree-round schedule on caller-built buckets (msmz_test.h): off / refs go to device buffers of this call, the
  // largest bucket into the meta block as the sort would have left it, then the engine's own plan_phase runs on them.  Everything the two kernels index
  // with is checked here first: they trust off, the chunk geometry and the capacities.
  int test_plan(const msmz_test_plan_args& a) override {
    if (TE) return MSMZ_ERR_UNSUPPORTED;
    constexpr uint32_t NB_CAP = 1u << 22, ENTRY_CAP = 1u << 25;
    if (!a.off || !a.meta || !a.desc || !a.bfin || a.nb == 0 || a.nb > NB_CAP) return MSMZ_ERR_ARG;
    if (a.tail_skip < 0 || a.tail_skip > 2 || a.chunk < 1 || a.chunk > (uint32_t)PLAN_CHUNK || a.chunk_top < 1 ||
        a.chunk_top > a.chunk || a.nb_main > a.nb)
      return MSMZ_ERR_ARG;
    const uint32_t nb = a.nb;
    if (a.off[0] != 0) return MSMZ_ERR_ARG;
    uint32_t max_bucket = 0;
    for (uint32_t g = 0; g < nb; g++) {
      if (a.off[g + 1] < a.off[g] || a.off[g + 1] > ENTRY_CAP) return MSMZ_ERR_ARG;
      const uint32_t sz = a.off[g + 1] - a.off[g];
      if (sz >= (1u << PLAN_RMAX)) return MSMZ_ERR_ARG;
      if (sz > max_bucket) max_bucket = sz;
    }
    const uint32_t n_entries = a.off[nb];
    if (n_entries && !a.refs) return MSMZ_ERR_ARG;
    for (uint32_t e = 0; e < n_entries; e++)
      if (a.refs[e] & LOC_ORIG) return MSMZ_ERR_ARG;   // bit 30 is the location words' "original point" flag
    // what the launches will write, from the same rule on the host
    const int R = plan_rounds(max_bucket, a.tail_skip);
    uint64_t total = 0;
    for (uint32_t g = 0; g < nb; g++) {
      const uint32_t sz = a.off[g + 1] - a.off[g];
      for (int r = 0; r < R && pairs_in_round(sz, r); r++) total += pairs_in_round(sz, r);
    }
    PlanChunks pc;
    pc.chunk = a.chunk;
    pc.nb_main = a.nb_main;
    pc.chunk_top = a.chunk_top;
    pc.n_main = (pc.nb_main + pc.chunk - 1) / pc.chunk;
    const uint32_t n_chunks = pc.n_main + (nb - pc.nb_main + pc.chunk_top - 1) / pc.chunk_top;
    if (a.desc_cap < total || a.bfin_cap < nb) return MSMZ_ERR_ARG;
    if (a.chunk_pairs && a.chunk_pairs_cap < (uint64_t)PLAN_RMAX * n_chunks) return MSMZ_ERR_ARG;

    MSMZ_HIP(hipSetDevice(eng_.device_));
    int st;
    DevBuf d_off, d_refs;   // (freed on every return)
    if ((st = d_off.ensure(((size_t)nb + 1) * 4)) || (st = d_refs.ensure(((size_t)n_entries + 1) * 4))) return st;
    MSMZ_HIP(hipMemcpyAsync(d_off.p, a.off, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, eng_.stream_));
    if (n_entries)
      MSMZ_HIP(hipMemcpyAsync(d_refs.p, a.refs, (size_t)n_entries * 4, hipMemcpyHostToDevice, eng_.stream_));
    MsmMeta hm;
    memset(&hm, 0, sizeof(hm));
    hm.max_bucket = max_bucket;   // (error = 0: as after a clean sort)
    MSMZ_HIP(hipMemcpyAsync(eng_.meta_.p, &hm, sizeof(hm), hipMemcpyHostToDevice, eng_.stream_));
    // Descriptor records: an MSM sizes them by its entries (pairs < entries); twice that here, so that a broken build
    // that numbers a round's pairs one chunk too far still writes inside the buffer.  Both outputs are filled with a
    // pattern that is no location, so a word the launch leaves unwritten cannot pass for one.
    const size_t desc_records = (size_t)2 * n_entries + 64;
    if ((st = eng_.desc_.ensure(desc_records * 8)) || (st = eng_.bfin_.ensure((size_t)nb * 16))) return st;
    MSMZ_HIP(hipMemsetAsync(eng_.desc_.p, 0xa5, desc_records * 8, eng_.stream_));
    MSMZ_HIP(hipMemsetAsync(eng_.bfin_.p, 0xa5, (size_t)nb * 16, eng_.stream_));
    msmz_opts opt;
    memset(&opt, 0, sizeof(opt));
    Run run = eng_.new_run(opt);
    if ((st = eng_.plan_phase(pc, d_off.as<uint32_t>(), d_refs.as<uint32_t>(), nb, a.tail_skip, desc_records, run))) return st;
    MSMZ_HIP(hipMemcpyAsync(a.meta, eng_.meta_.p, sizeof(MsmMeta), hipMemcpyDeviceToHost, eng_.stream_));
    if (total) MSMZ_HIP(hipMemcpyAsync(a.desc, eng_.desc_.p, (size_t)total * 8, hipMemcpyDeviceToHost, eng_.stream_));
    MSMZ_HIP(hipMemcpyAsync(a.bfin, eng_.bfin_.p, (size_t)nb * 16, hipMemcpyDeviceToHost, eng_.stream_));
    if (a.chunk_pairs)
      MSMZ_HIP(hipMemcpyAsync(a.chunk_pairs, eng_.rscan_.p, (size_t)PLAN_RMAX * n_chunks * 4, hipMemcpyDeviceToHost, eng_.stream_));
    MSMZ_HIP(hipStreamSynchronize(eng_.stream_));
    return MSMZ_OK;
  }

 private:
  Staging staging() const { return Staging{eng_.device_, eng_.stream_, eng_.stage_}; }

  // The operands of the tree rounds as test_batch_add and the LOCATIONS mode of test_reduce take them (Weierstrass):
  // d_pts <- the np canonical points in the resident format of an MSM; slots_ <- records 0 .. recs - 1 in whole groups
  // of 64, filled with a pattern that decodes to no result (so a record a launch leaves unwritten cannot pass for one),
  // then the ns canonical slot records.  A coordinate >= p raises the meta error word, which the caller has cleared.
  int load_operands(DevBuf& d_pts, const uint32_t* d_pxy, const uint8_t* d_pinf, size_t np, const uint32_t* d_sxy,
                    const uint8_t* d_sinf, size_t ns, uint32_t recs) {
    int st;
    if ((st = d_pts.ensure((np ? np : 1) * E::PW_WORDS * 4))) return st;
    if ((st = eng_.slots_.ensure(((size_t)recs + 64) * SlotFmt<F>::WORDS * 4))) return st;
    MSMZ_HIP(hipMemsetAsync(eng_.slots_.p, 0xa5, slot_words<F>((recs + 63u) & ~63u) * 4, eng_.stream_));
    uint32_t* d_error = &eng_.meta_.template as<MsmMeta>()->error;
    if constexpr (!TE) {
      if (np)
        hipLaunchKernelGGL((k_points_to_resident<P>), dim3((np + 255) / 256), dim3(256), 0, eng_.stream_, d_pts.as<uint32_t>(),
                           d_pxy, d_pinf, (uint32_t)np, 0, d_error);
      if (ns)
        hipLaunchKernelGGL((k_test_slots_in<F>), dim3((ns + 255) / 256), dim3(256), 0, eng_.stream_,
                           eng_.slots_.template as<uint32_t>(), d_sxy, d_sinf, (uint32_t)ns, d_error);
    }
    return MSMZ_OK;
  }

  E& eng_;
};

}  // namespace msmz
