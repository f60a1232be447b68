// block_pattern.cpp -- see block_pattern.hpp.
#include "block_pattern.hpp"


#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <unordered_map>

#include "common.hpp"

namespace mha {
namespace {

// role record (kBpRoleInts ints)
enum { R_EREC_LO = 0, R_EREC_HI, R_ESTRIDE, R_ROWB_LO, R_ROWB_HI, R_NRUNS, R_NBLOCKS, R_COST, R_WOFF_LO, R_WOFF_HI,
       R_WDOUBLES, R_PATTERN, R_NELEMS };
// part header (kBpHdrInts ints)
enum { H_WOFF = 0, H_KS, H_NCT, H_LEN, H_CT0, H_NTILE, H_FLAGS, H_CLASS, H_MASK0, H_MASK1, H_MASK2 };  // flags: 1 rows of fixed dofs, 2 a plain tail tile follows the group, 4 / 8 / 16 trim class (see the mask loop)

uint64_t fnv1a(const std::vector<uint8_t> &b) {
  uint64_t h = 1469598103934665603ull;
  for (uint8_t c : b) { h ^= c; h *= 1099511628211ull; }
  return h;
}

inline void put16(std::vector<uint8_t> &o, int v) { o.push_back(v & 0xff); o.push_back((v >> 8) & 0xff); }
inline void put24(std::vector<uint8_t> &o, int v) { put16(o, v); o.push_back((v >> 16) & 0xff); }

// Everything the kernel's static tables depend on, as bytes: rows (length, fixed), touched elements (count) and per
// contribution pair the owned row, the element, the local dof and the slot of every column of that element.
void block_signature(const RowBlocks &rb, int b, int n, const int32_t *rowptr, const uint8_t *fixed, const uint8_t *slot,
                     int slot_bytes, std::vector<uint8_t> &out) {
  out.clear();
  const int r0 = rb.row_ptr[b], R = rb.row_ptr[b + 1] - r0;
  const int t0 = rb.elem_ptr[b], T = rb.elem_ptr[b + 1] - t0;
  put16(out, R);
  put16(out, T);
  for (int o = 0; o < R; ++o) {
    const int r = rb.rows[r0 + o];
    put24(out, rowptr[r + 1] - rowptr[r]);
    out.push_back((fixed && fixed[r]) ? 1 : 0);
    out.push_back((o > 0 && rb.rows[r0 + o - 1] + 1 == r) ? 0 : 1);  // 1: the row starts a new run of consecutive rows
  }
  for (int p = rb.pair_ptr[b]; p < rb.pair_ptr[b + 1]; ++p) {
    const uint32_t pk = rb.pairs[p];
    const int o = pk >> 16, t = (pk >> 8) & 0xff, si = pk & 0xff;
    put16(out, o);
    out.push_back(static_cast<uint8_t>(t));
    out.push_back(static_cast<uint8_t>(si));
    const uint8_t *s = slot + (static_cast<size_t>(rb.elems[t0 + t]) * n + si) * n * slot_bytes;
    out.insert(out.end(), s, s + static_cast<size_t>(n) * slot_bytes);
  }
}

struct Inc { int si, t; const uint8_t *slots; };

struct RowClass {
  int len = 0, ni = 0;
  bool fixed = false;
  std::vector<int> inst_row;             // block-local rows of the instances
  std::vector<std::vector<int>> inst_t;  // per instance: block-local element of incidence k
  std::vector<int> si;                   // local dof of incidence k
  std::vector<std::vector<int>> slots;   // per incidence k: slot of every column of that element
  int ks = 0, nct = 0, stride = 0, w_doubles = 0;
  int bin = 0, w_off = 0;                // role (LDS bin) and offset inside it
};

inline int stride_for(int nct) { return (nct % 2 == 1) ? 16 * nct : 16 * nct + 16; }

}  // namespace

BlockPatternPlan build_block_patterns(const RowBlocks &rb, int n, int nsym, const int32_t *rowptr, const uint8_t *fixed,
                                      const void *elem_slot, int slot_bytes, const double *khat, int num_cus,
                                      size_t lds_budget_bytes, int max_patterns) {
  BlockPatternPlan pl;
  pl.nsym = nsym;
  pl.ke = nsym + 1;
  const int ke = pl.ke;
  const uint8_t *slot = static_cast<const uint8_t *>(elem_slot);
  auto fail = [&](const std::string &m) { pl.usable = false; pl.why = m; return pl; };
  if (rb.num_blocks == 0) return fail("no row blocks");
  if (ke > kBpRecDoubles) return fail("more geometry components than an element record holds");
  const size_t nn = static_cast<size_t>(n) * n;

  // ---- 1. pattern of every block ----
  std::unordered_map<uint64_t, std::vector<int32_t>> by_hash;  // hash -> pattern ids (collisions resolved by comparing bytes)
  std::vector<int32_t> rep;                                    // representative block of each pattern
  std::vector<std::vector<int32_t>> members;
  std::vector<uint8_t> cur, other;
  for (int b = 0; b < rb.num_blocks; ++b) {
    block_signature(rb, b, n, rowptr, fixed, slot, slot_bytes, cur);
    std::vector<int32_t> &ids = by_hash[fnv1a(cur)];
    int found = -1;
    for (int id : ids) {
      block_signature(rb, rep[id], n, rowptr, fixed, slot, slot_bytes, other);
      if (other == cur) { found = id; break; }
    }
    if (found < 0) {
      found = static_cast<int>(rep.size());
      if (found >= max_patterns) return fail("row blocks share too few assembly patterns (unstructured numbering)");
      rep.push_back(b);
      members.emplace_back();
      ids.push_back(found);
    }
    members[found].push_back(b);
  }
  pl.num_patterns = static_cast<int>(rep.size());

  // ---- 2. per pattern: classes, tiles, parts, roles ----
  struct RoleBuild {
    int pattern, bin, R, T, nruns;
    int w_doubles = 0;
    int64_t w_off = 0;             // start of the role's LDS image inside pl.w
    int64_t cost = 0;              // per block
    std::vector<std::vector<int32_t>> wave_parts;  // [kBpWaves] -> part indices (global)
  };
  std::vector<RoleBuild> roles;
  const int budget_doubles = static_cast<int>(lds_budget_bytes / sizeof(double));

  for (int pat = 0; pat < pl.num_patterns; ++pat) {
    const int b = rep[pat];
    const int r0 = rb.row_ptr[b], R = rb.row_ptr[b + 1] - r0;
    const int t0 = rb.elem_ptr[b], T = rb.elem_ptr[b + 1] - t0;
    if ((T + 1) * kBpRecDoubles > 512) return fail("a block touches more elements than the record loader fetches (63)");
    pl.max_rec_doubles = std::max(pl.max_rec_doubles, (T + 1) * kBpRecDoubles);
    // runs of consecutive rows: contiguous in the CRS value array, so one offset per (block, run) locates every row
    std::vector<int> run_of(R), run_first;
    for (int o = 0; o < R; ++o) {
      if (o == 0 || rb.rows[r0 + o - 1] + 1 != rb.rows[r0 + o]) run_first.push_back(o);
      run_of[o] = static_cast<int>(run_first.size()) - 1;
      if (rowptr[rb.rows[r0 + o]] - rowptr[rb.rows[r0 + run_first.back()]] >= (1 << 20)) return fail("a run of rows is longer than 2^20 entries");
    }
    const int nruns = static_cast<int>(run_first.size());
    if (nruns > kBpSegInts || nruns >= 2048) return fail("the rows of a block form too many runs");
    // incidences of every owned row
    std::vector<std::vector<Inc>> inc(R);
    for (int p = rb.pair_ptr[b]; p < rb.pair_ptr[b + 1]; ++p) {
      const uint32_t pk = rb.pairs[p];
      const int o = pk >> 16, t = (pk >> 8) & 0xff, si = pk & 0xff;
      inc[o].push_back({si, t, slot + (static_cast<size_t>(rb.elems[t0 + t]) * n + si) * n * slot_bytes});
    }
    std::map<std::vector<uint8_t>, int> class_of;
    std::vector<RowClass> classes;
    std::vector<uint8_t> key;
    for (int o = 0; o < R; ++o) {
      const int r = rb.rows[r0 + o];
      const int len = rowptr[r + 1] - rowptr[r];
      const bool fx = fixed && fixed[r];
      std::vector<Inc> &v = inc[o];
      const size_t sb = static_cast<size_t>(n) * slot_bytes;
      std::sort(v.begin(), v.end(), [&](const Inc &a, const Inc &c) {
        if (a.si != c.si) return a.si < c.si;
        return std::memcmp(a.slots, c.slots, sb) < 0;
      });
      key.clear();
      put24(key, len);
      key.push_back(fx ? 1 : 0);
      if (!fx)
        for (const Inc &i : v) { key.push_back(static_cast<uint8_t>(i.si)); key.insert(key.end(), i.slots, i.slots + sb); }
      auto it = class_of.find(key);
      int c;
      if (it == class_of.end()) {
        c = static_cast<int>(classes.size());
        class_of[key] = c;
        RowClass rc;
        rc.len = len;
        rc.fixed = fx;
        rc.ni = fx ? 0 : static_cast<int>(v.size());
        if (!fx)
          for (const Inc &i : v) {
            rc.si.push_back(i.si);
            std::vector<int> s(n);
            for (int sj = 0; sj < n; ++sj)
              s[sj] = slot_bytes == 1 ? i.slots[sj] : reinterpret_cast<const uint16_t *>(i.slots)[sj];
            rc.slots.push_back(std::move(s));
          }
        rc.nct = (len + 15) / 16;
        rc.stride = stride_for(rc.nct);
        rc.ks = (rc.ni * ke + 3) / 4;
        if (rc.ks > kBpMaxKSteps) return fail("a dof is shared by more elements than the pattern kernel holds");
        rc.w_doubles = rc.ks * 4 * rc.stride;
        if (rc.w_doubles > budget_doubles) return fail("a pattern matrix does not fit the LDS");
        classes.push_back(std::move(rc));
      } else {
        c = it->second;
      }
      classes[c].inst_row.push_back(o);
      std::vector<int> ts;
      if (!fx)
        for (const Inc &i : v) ts.push_back(i.t);
      classes[c].inst_t.push_back(std::move(ts));
    }
    // LDS bins: first fit, largest W first
    std::vector<int> order(classes.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return classes[a].w_doubles > classes[c].w_doubles; });
    std::vector<int> bin_fill;
    for (int c : order) {
      RowClass &rc = classes[c];
      int bin = -1;
      for (size_t k = 0; k < bin_fill.size() && bin < 0; ++k)
        if (bin_fill[k] + rc.w_doubles <= budget_doubles) bin = static_cast<int>(k);
      if (bin < 0) { bin = static_cast<int>(bin_fill.size()); bin_fill.push_back(0); }
      rc.bin = bin;
      rc.w_off = bin_fill[bin];
      bin_fill[bin] += rc.w_doubles;
    }
    if (bin_fill.empty()) bin_fill.push_back(0);
    const int first_role = static_cast<int>(roles.size());
    std::vector<size_t> role_woff(bin_fill.size());
    for (size_t k = 0; k < bin_fill.size(); ++k) {
      role_woff[k] = pl.w.size();
      pl.w.resize(pl.w.size() + 2 * static_cast<size_t>(bin_fill[k]), 0.0);  // stiffness rows | mass rows
      pl.max_w_doubles = std::max(pl.max_w_doubles, bin_fill[k]);
      RoleBuild rbld;
      rbld.pattern = pat;
      rbld.bin = static_cast<int>(k);
      rbld.R = R;
      rbld.T = T;
      rbld.nruns = nruns;
      rbld.w_doubles = bin_fill[k];
      rbld.w_off = static_cast<int64_t>(role_woff[k]);
      rbld.wave_parts.assign(kBpWaves, {});
      roles.push_back(std::move(rbld));
    }
    // W images
    for (RowClass &rc : classes) {
      if (rc.fixed) continue;
      double *W = pl.w.data() + role_woff[rc.bin] + rc.w_off;
      const size_t mass = static_cast<size_t>(bin_fill[rc.bin]);  // offset of the mass half of the role's image
      for (int k = 0; k < rc.ni; ++k)
        for (int sj = 0; sj < n; ++sj)
          for (int m = 0; m < ke; ++m)
            W[(m == nsym ? mass : 0) + static_cast<size_t>(k * ke + m) * rc.stride + rc.slots[k][sj]] +=
                khat[m * nn + static_cast<size_t>(rc.si[k]) * n + sj];
    }
    // tiles of 16 instances, cut into UNITS of up to four column tiles (what one wavefront computes and stores per
    // block: the products of a unit are transposed so that every store writes 64 consecutive entries of one row); a
    // single left-over tile rides with the group before it, two or three form a unit of their own.  All wavefronts of
    // a workgroup work on the same block at the same time (the rows of a block are neighbours in memory: written
    // within microseconds of each other they leave the L2 as whole DRAM pages), so the units -- not blocks -- are what
    // is dealt to the wavefronts, heaviest first.
    struct Tile { int cls, tile; int64_t cost; };
    std::vector<std::vector<Tile>> tiles(bin_fill.size());
    for (size_t c = 0; c < classes.size(); ++c) {
      const RowClass &rc = classes[c];
      const int ntile = (static_cast<int>(rc.inst_row.size()) + 15) / 16;
      for (int t = 0; t < ntile; ++t)
        tiles[rc.bin].push_back({static_cast<int>(c), t, static_cast<int64_t>(rc.nct) * (rc.ks + 4)});
    }
    for (size_t k = 0; k < bin_fill.size(); ++k) {
      RoleBuild &role = roles[first_role + k];
      int64_t total = 0;
      for (const Tile &t : tiles[k]) total += t.cost;
      role.cost = total;
      struct PartBuild { int cls, tile, ct0, ntile, tail; double cost; };
      std::vector<PartBuild> parts;
      for (const Tile &t : tiles[k]) {
        const RowClass &rc = classes[t.cls];
        const int ng = rc.nct / 4, rem = rc.nct % 4;
        for (int g = 0; g < ng; ++g) {
          const int tail = (g == ng - 1 && rem == 1) ? 1 : 0;
          parts.push_back({t.cls, t.tile, 4 * g, 4, tail, static_cast<double>((4 + tail) * (rc.ks + 1))});
        }
        if (ng == 0 && rem == 1) parts.push_back({t.cls, t.tile, 0, 0, 1, static_cast<double>(rc.ks + 1)});
        if (rem >= 2) parts.push_back({t.cls, t.tile, 4 * ng, rem, 0, static_cast<double>(rem * (rc.ks + 1) + 2)});
      }
      // cost of a product unit = its non-zero 4 x 16 blocks of W (the products the kernel's trimmed forms issue)
      for (PartBuild &pb : parts) {
        const RowClass &rc = classes[pb.cls];
        if (rc.fixed) continue;
        const double *Wk = pl.w.data() + role_woff[rc.bin] + rc.w_off, *Wm = Wk + bin_fill[rc.bin];
        int nzb = 0;
        for (int sidx = 0; sidx < rc.ks; ++sidx)
          for (int q = 0; q < pb.ntile + pb.tail; ++q) {
            bool any = false;
            for (int r = 4 * sidx; r < 4 * sidx + 4 && !any; ++r)
              for (int lc = 0; lc < 16 && !any; ++lc) {
                const int cc = bp_unit_col(pb.ct0, pb.ntile, q, lc);
                any = Wk[static_cast<size_t>(r) * rc.stride + cc] != 0.0 || Wm[static_cast<size_t>(r) * rc.stride + cc] != 0.0;
              }
            nzb += any ? 1 : 0;
          }
        pb.cost = nzb + 1;
      }
      std::stable_sort(parts.begin(), parts.end(), [](const PartBuild &a, const PartBuild &c) { return a.cost > c.cost; });
      // units of fixed rows (zeros, no products) go to wavefronts that carry no products when there are any: the
      // kernel's fast forms take wavefronts whose units are all of one kind
      std::stable_partition(parts.begin(), parts.end(), [&](const PartBuild &a) { return !classes[a.cls].fixed; });
      std::vector<double> load(kBpWaves, 0.0), simd_load(4, 0.0);
      std::vector<char> has_products(kBpWaves, 0);
      for (const PartBuild &pb : parts) {
        int wv = -1;
        if (classes[pb.cls].fixed) {
          for (int w = 0; w < kBpWaves; ++w)
            if (!has_products[w] && (wv < 0 || load[w] < load[wv])) wv = w;
        }
        if (wv < 0) {
          // a product unit: a wavefront of its own while there are free ones, on the SIMD (wavefront id mod 4: the four
          // SIMDs of a CU take a workgroup's wavefronts round robin) whose matrix pipe has the least work so far
          for (int w = 0; w < kBpWaves; ++w)
            if (load[w] == 0.0 && (wv < 0 || simd_load[w % 4] < simd_load[wv % 4])) wv = w;
          if (wv < 0) wv = static_cast<int>(std::min_element(load.begin(), load.end()) - load.begin());
          simd_load[wv % 4] += pb.cost;
        }
        load[wv] += pb.cost;
        if (!classes[pb.cls].fixed) has_products[wv] = 1;
        const RowClass &rc = classes[pb.cls];
        const int pidx = pl.num_parts++;
        role.wave_parts[wv].push_back(pidx);
        int32_t hdr[kBpHdrInts] = {0};
        hdr[H_WOFF] = rc.w_off;
        hdr[H_KS] = rc.ks;
        hdr[H_NCT] = rc.nct;
        hdr[H_LEN] = rc.len;
        hdr[H_CT0] = pb.ct0;
        hdr[H_NTILE] = pb.ntile;
        hdr[H_FLAGS] = (rc.fixed ? 1 : 0) | (pb.tail ? 2 : 0);
        hdr[H_CLASS] = pl.num_classes + pb.cls;
        if (!rc.fixed) {  // which 4 x 16 blocks of the unit's part of W hold anything: the kernel skips the products of the others
          const double *Wk = pl.w.data() + role_woff[rc.bin] + rc.w_off, *Wm = Wk + bin_fill[rc.bin];
          for (int sidx = 0; sidx < rc.ks; ++sidx)
            for (int q = 0; q < pb.ntile + pb.tail; ++q) {
              bool any = false;
              for (int r = 4 * sidx; r < 4 * sidx + 4 && !any; ++r)
                for (int lc = 0; lc < 16 && !any; ++lc) {
                  const int cc = bp_unit_col(pb.ct0, pb.ntile, q, lc);
                  any = Wk[static_cast<size_t>(r) * rc.stride + cc] != 0.0 || Wm[static_cast<size_t>(r) * rc.stride + cc] != 0.0;
                }
              const int bit = sidx * 5 + q;
              if (any) hdr[H_MASK0 + bit / 32] |= static_cast<int32_t>(1u << (bit % 32));
            }
          // trim class of a unit of two tile pairs (flags bits 2..4, read by the kernel's specialised form): the first pair
          // (classes 1, 3) or the second (2, 4) has only zero blocks in the second (1, 4) or first (2, 3) half of the k-steps
          const int nq = pb.ntile + pb.tail;
          if (nq >= 2 && rc.ks >= 2) {
            bool t[5] = {false, true, true, true, true};
            if (pb.ntile != 4 || pb.tail) t[1] = t[2] = t[3] = t[4] = false;
            for (int sidx = 0; sidx < rc.ks; ++sidx)
              for (int q = 0; q < nq; ++q) {
                const int bit = sidx * 5 + q;
                const bool nz = (static_cast<uint32_t>(hdr[H_MASK0 + bit / 32]) >> (bit % 32)) & 1u;
                if (!nz) continue;
                const bool second = sidx >= rc.ks / 2;
                if (q < 2 && second) t[1] = false;
                if (q >= 2 && !second) t[2] = false;
                if (q < 2 && !second) t[3] = false;
                if (q >= 2 && second) t[4] = false;
              }
            for (int k = 1; k <= 4; ++k)
              if (t[k]) { hdr[H_FLAGS] |= k << 2; break; }
          }
        }
        pl.part_hdr.insert(pl.part_hdr.end(), hdr, hdr + kBpHdrInts);
        const size_t base = pl.part_lane.size();
        pl.part_lane.resize(base + static_cast<size_t>(kBpLaneRows) * 64, 0);
        int32_t *L = pl.part_lane.data() + base;
        const int ninst = static_cast<int>(rc.inst_row.size());
        const int zero_off = T * kBpRecDoubles;
        for (int lane = 0; lane < 64; ++lane) {
          const int i = lane & 15, kk = lane >> 4;
          const int inst = pb.tile * 16 + i;
          for (int s = 0; s < kBpMaxKSteps; ++s) {
            const int kidx = 4 * s + kk;
            int off = zero_off;
            if (inst < ninst && !rc.fixed && kidx < rc.ni * ke) {
              const int kel = kidx / ke, m = kidx % ke;
              off = rc.inst_t[inst][kel] * kBpRecDoubles + m;
            }
            L[s * 64 + lane] = off;
          }
          for (int t = 0; t < 4; ++t) {
            const int r = kk + 4 * t;  // result register t of this lane belongs to tile row (lane >> 4) + 4 t
            const int instr = pb.tile * 16 + r;
            // run of consecutive rows the result row lies in and its CRS offset relative to the run's first row
            // (both part of the pattern), -1 = no row
            int packed = -1;
            if (instr < ninst) {
              const int o = rc.inst_row[instr];
              packed = (run_of[o] << 20) | (rowptr[rb.rows[r0 + o]] - rowptr[rb.rows[r0 + run_first[run_of[o]]]]);
            }
            L[(16 + t) * 64 + lane] = packed;
          }
          {  // the same for tile row (lane & 15): what the row-contiguous stores of the kernel consult
            const int instr = pb.tile * 16 + i;
            int packed = -1;
            if (instr < ninst) {
              const int o = rc.inst_row[instr];
              packed = (run_of[o] << 20) | (rowptr[rb.rows[r0 + o]] - rowptr[rb.rows[r0 + run_first[run_of[o]]]]);
            }
            L[20 * 64 + lane] = packed;
          }
        }
      }
    }
    // wave 0 also fetches the element records, which the kernel builds only into its shapes of at most three chains:
    // give it such a unit (from the same SIMD if there is one: wavefront id mod 4)
    for (size_t k = 0; k < bin_fill.size(); ++k) {
      RoleBuild &role = roles[first_role + k];
      auto chains = [&](int wv) {  // of a wavefront that owns exactly one product unit, else 0
        if (role.wave_parts[wv].size() != 1) return 0;
        const int32_t *h = &pl.part_hdr[static_cast<size_t>(role.wave_parts[wv][0]) * kBpHdrInts];
        return (h[H_FLAGS] & 1) ? 0 : h[H_NTILE] + ((h[H_FLAGS] & 2) ? 1 : 0);
      };
      if (role.wave_parts[0].empty() || chains(0) <= 3) continue;
      int best = -1;
      for (int wv = 1; wv < kBpWaves; ++wv) {
        const int nc = chains(wv);
        if (nc < 1 || nc > 3) continue;
        if (best < 0 || (wv % 4 == 0 && best % 4 != 0)) best = wv;
      }
      if (best > 0) std::swap(role.wave_parts[0], role.wave_parts[best]);
    }
    pl.num_classes += static_cast<int>(classes.size());
  }

  // ---- 3. (workgroups are cut after the block tables: step 5) ----
  pl.num_roles = static_cast<int>(roles.size());

  // ---- 4. role records, block-major tables ----
  pl.role.assign(static_cast<size_t>(pl.num_roles) * kBpRoleInts, 0);
  pl.part_ptr.assign(static_cast<size_t>(pl.num_roles) * (kBpWaves + 1), 0);
  // parts must be contiguous per (role, wave): renumber
  {
    std::vector<int32_t> new_hdr, new_lane;
    new_hdr.reserve(pl.part_hdr.size());
    new_lane.reserve(pl.part_lane.size());
    int next = 0;
    for (int k = 0; k < pl.num_roles; ++k)
      for (int wv = 0; wv <= kBpWaves; ++wv) {
        pl.part_ptr[static_cast<size_t>(k) * (kBpWaves + 1) + wv] = next;
        if (wv == kBpWaves) break;
        for (int pidx : roles[k].wave_parts[wv]) {
          new_hdr.insert(new_hdr.end(), pl.part_hdr.begin() + static_cast<size_t>(pidx) * kBpHdrInts,
                         pl.part_hdr.begin() + static_cast<size_t>(pidx + 1) * kBpHdrInts);
          new_lane.insert(new_lane.end(), pl.part_lane.begin() + static_cast<size_t>(pidx) * kBpLaneRows * 64,
                          pl.part_lane.begin() + static_cast<size_t>(pidx + 1) * kBpLaneRows * 64);
          ++next;
        }
      }
    pl.part_hdr.swap(new_hdr);
    pl.part_lane.swap(new_lane);
  }
  // ---- 5. persistent workgroups, exactly one per CU: the role-major block sequence is cut into num_cus contiguous
  //         pieces of equal cost; a piece that crosses a role boundary becomes several SEGMENTS (the workgroup reloads
  //         the LDS image between them), so small roles cost no extra workgroup and nobody waits for a free CU.
  //         Starting a role costs about three blocks (image load, pipeline fill), continuing it in a new segment one ----
  {
    const int nwg = std::max(1, num_cus);
    auto block_cost = [&](int k) { return static_cast<double>(std::max<int64_t>(1, roles[k].cost)); };
    double total_cost = 0.0;
    for (int k = 0; k < pl.num_roles; ++k) total_cost += (static_cast<double>(members[roles[k].pattern].size()) + 3.0) * block_cost(k);
    for (double target = total_cost / nwg;; target *= 1.02) {
      pl.seg.clear();
      pl.wg_seg_ptr.assign(1, 0);
      int wg = 0;
      double load = 0.0;  // of the current workgroup
      int last_role = -1;
      bool fits = true;
      for (int k = 0; k < pl.num_roles && fits; ++k) {
        const double c = block_cost(k);
        const int nb = static_cast<int>(members[roles[k].pattern].size());
        const int seg_cap = std::max(1, kBpSegInts / roles[k].nruns);
        int first = 0;
        while (first < nb) {
          const double start = (last_role == k ? 1.0 : 3.0) * c;
          int take = static_cast<int>(std::floor((target - load - start) / c + 0.5));
          if (take < 1 && load > 0.0) {  // no room for another segment: next workgroup
            if (wg == nwg - 1) { fits = false; break; }
            pl.wg_seg_ptr.push_back(static_cast<int32_t>(pl.seg.size() / 4));
            ++wg;
            load = 0.0;
            last_role = -1;
            continue;
          }
          take = std::max(1, std::min(std::min(take, nb - first), seg_cap));
          pl.seg.push_back(k);
          pl.seg.push_back(first);
          pl.seg.push_back(take);
          pl.seg.push_back(0);
          first += take;
          load += start + take * c;
          last_role = k;
        }
      }
      if (fits) {
        while (static_cast<int>(pl.wg_seg_ptr.size()) < nwg + 1) pl.wg_seg_ptr.push_back(static_cast<int32_t>(pl.seg.size() / 4));
        pl.wg_seg_ptr.back() = static_cast<int32_t>(pl.seg.size() / 4);
        break;
      }
    }
    pl.num_wgs = nwg;
  }
  // ---- 5b. order of a role's blocks inside its block-major tables.  A workgroup walks a contiguous range of them
  //          (its segment), one block at a time, and all workgroups run at about the same pace: the t-th blocks of all
  //          segments are written at about the same time.  They are made NEIGHBOURS IN THE CRS VALUE ARRAY (blocks sorted
  //          by the offset of their first row, dealt round robin over the role's segments): the ~256 x 64 KB in flight
  //          then cover a few contiguous megabytes instead of 4096 scattered row runs, which is what the memory's
  //          row buffers need (measured: the stores alone took 336 us for 1.08 GB with every workgroup in a region of
  //          its own). ----
  std::vector<std::vector<int32_t>> role_blocks(pl.num_roles);
  {
    std::vector<std::vector<std::pair<int, int>>> segs(pl.num_roles);  // per role: (first, blocks) of its segments
    for (size_t sg = 0; sg < pl.seg.size() / 4; ++sg) segs[pl.seg[4 * sg]].push_back({pl.seg[4 * sg + 1], pl.seg[4 * sg + 2]});
    for (int k = 0; k < pl.num_roles; ++k) {
      std::vector<int32_t> sorted = members[roles[k].pattern];
      std::stable_sort(sorted.begin(), sorted.end(), [&](int32_t x, int32_t y) { return rb.row_base[rb.row_ptr[x]] < rb.row_base[rb.row_ptr[y]]; });
      std::vector<int32_t> &out = role_blocks[k];
      out.assign(sorted.size(), -1);
      size_t next = 0;
      int longest = 0;
      for (const auto &sg : segs[k]) longest = std::max(longest, sg.second);
      for (int t = 0; t < longest; ++t)
        for (const auto &sg : segs[k])
          if (t < sg.second) out[static_cast<size_t>(sg.first) + t] = sorted[next++];
      if (next != sorted.size()) return fail("the segments of a role do not cover its blocks");
    }
  }
  for (int k = 0; k < pl.num_roles; ++k) {
    const RoleBuild &r = roles[k];
    const std::vector<int32_t> &blocks = role_blocks[k];
    int32_t *ro = &pl.role[static_cast<size_t>(k) * kBpRoleInts];
    const int64_t erec_base = static_cast<int64_t>(pl.erec_elem.size());
    const int64_t row_base = static_cast<int64_t>(pl.rowbase.size());
    ro[R_EREC_LO] = static_cast<int32_t>(erec_base & 0xffffffffll);
    ro[R_EREC_HI] = static_cast<int32_t>(erec_base >> 32);
    ro[R_ESTRIDE] = r.T + 1;
    ro[R_ROWB_LO] = static_cast<int32_t>(row_base & 0xffffffffll);
    ro[R_ROWB_HI] = static_cast<int32_t>(row_base >> 32);
    ro[R_NRUNS] = r.nruns;
    ro[R_NBLOCKS] = static_cast<int32_t>(blocks.size());
    ro[R_COST] = static_cast<int32_t>(std::min<int64_t>(r.cost, 0x7fffffff));
    ro[R_WOFF_LO] = static_cast<int32_t>(r.w_off & 0xffffffffll);
    ro[R_WOFF_HI] = static_cast<int32_t>(r.w_off >> 32);
    ro[R_WDOUBLES] = r.w_doubles;
    ro[R_PATTERN] = r.pattern;
    ro[R_NELEMS] = r.T;
    pl.role_runlen_off.push_back(static_cast<int64_t>(pl.runlen.size()));
    if (!blocks.empty()) {  // entries of every run, from the role's first block (the pattern fixes them)
      const int32_t b0 = blocks[0];
      for (int o = rb.row_ptr[b0]; o < rb.row_ptr[b0 + 1]; ++o) {
        if (o == rb.row_ptr[b0] || rb.rows[o - 1] + 1 != rb.rows[o]) pl.runlen.push_back(0);
        pl.runlen.back() += rowptr[rb.rows[o] + 1] - rowptr[rb.rows[o]];
      }
    }
    for (int32_t b : blocks) {
      for (int t = rb.elem_ptr[b]; t < rb.elem_ptr[b + 1]; ++t) pl.erec_elem.push_back(rb.elems[t]);
      pl.erec_elem.push_back(-1);
      for (int o = rb.row_ptr[b]; o < rb.row_ptr[b + 1]; ++o)  // CRS offset of the first row of every run
        if (o == rb.row_ptr[b] || rb.rows[o - 1] + 1 != rb.rows[o]) pl.rowbase.push_back(rb.row_base[o]);
    }
    int64_t mf = 0;
    for (int wv = 0; wv < kBpWaves; ++wv)
      for (int p = pl.part_ptr[static_cast<size_t>(k) * (kBpWaves + 1) + wv]; p < pl.part_ptr[static_cast<size_t>(k) * (kBpWaves + 1) + wv + 1]; ++p) {
        const int32_t *h = &pl.part_hdr[static_cast<size_t>(p) * kBpHdrInts];
        int bits = 0;
        for (int wd = 0; wd < 3; ++wd) bits += __builtin_popcount(static_cast<uint32_t>(h[H_MASK0 + wd]));
        mf += static_cast<int64_t>(bits) * static_cast<int64_t>(blocks.size());
      }
    pl.mfma_per_assembly += mf;
  }
  pl.usable = true;
  return pl;
}

void block_patterns_host_apply(const BlockPatternPlan &pl, const double *factors, double su, double st, bool overwrite,
                               double *vals) {
  MHA_REQUIRE(pl.usable, MHA_ERR_STATE, "block patterns not usable: " << pl.why);
  const int ke = pl.ke;
  std::vector<double> rec;
  for (int wg = 0; wg < pl.num_wgs; ++wg)
  for (int sg = pl.wg_seg_ptr[wg]; sg < pl.wg_seg_ptr[wg + 1]; ++sg) {
    const int role = pl.seg[4 * sg], first = pl.seg[4 * sg + 1], nseg = pl.seg[4 * sg + 2];
    const int32_t *ro = &pl.role[static_cast<size_t>(role) * kBpRoleInts];
    const int64_t erec_base = (static_cast<int64_t>(ro[R_EREC_HI]) << 32) | static_cast<uint32_t>(ro[R_EREC_LO]);
    const int64_t row_base = (static_cast<int64_t>(ro[R_ROWB_HI]) << 32) | static_cast<uint32_t>(ro[R_ROWB_LO]);
    const int estride = ro[R_ESTRIDE], nruns = ro[R_NRUNS];
    MHA_REQUIRE(first >= 0 && first + nseg <= ro[R_NBLOCKS], MHA_ERR_STATE, "segment outside its role");
    const double *Wrole = pl.w.data() + ((static_cast<int64_t>(ro[R_WOFF_HI]) << 32) | static_cast<uint32_t>(ro[R_WOFF_LO]));
    for (int wv = 0; wv < kBpWaves; ++wv)
      for (int p = pl.part_ptr[static_cast<size_t>(role) * (kBpWaves + 1) + wv]; p < pl.part_ptr[static_cast<size_t>(role) * (kBpWaves + 1) + wv + 1]; ++p) {
        const int32_t *h = &pl.part_hdr[static_cast<size_t>(p) * kBpHdrInts];
        const int32_t *L = &pl.part_lane[static_cast<size_t>(p) * kBpLaneRows * 64];
        const int ks = h[H_KS], nct = h[H_NCT], len = h[H_LEN], stride = stride_for(nct);
        const bool fixed_class = h[H_FLAGS] & 1;
        if (fixed_class && !overwrite) continue;
        const double *W = Wrole + h[H_WOFF], *Wm = W + ro[R_WDOUBLES];
        const int c_begin = 16 * h[H_CT0], c_end = std::min(len, 16 * (h[H_CT0] + h[H_NTILE] + ((h[H_FLAGS] & 2) ? 1 : 0)));
        for (int i = 0; i < nseg; ++i) {
          const int64_t j = first + i;
          // the block's element records, as build_erec2_kernel lays them out
          rec.assign(static_cast<size_t>(estride) * kBpRecDoubles, 0.0);
          for (int t = 0; t < estride; ++t) {
            const int e = pl.erec_elem[static_cast<size_t>(erec_base + j * estride + t)];
            if (e >= 0)
              for (int m = 0; m < ke; ++m) rec[static_cast<size_t>(t) * kBpRecDoubles + m] = factors[static_cast<size_t>(e) * ke + m];
          }
          for (int row = 0; row < 16; ++row) {
            // result rows live in lanes (row & 3) << 4 .. with register t = row >> 2
            const int packed = L[(16 + (row >> 2)) * 64 + ((row & 3) << 4)];
            MHA_REQUIRE(packed == L[20 * 64 + row] && packed == L[20 * 64 + 48 + row], MHA_ERR_STATE, "row tables of a part disagree");
            if (packed < 0) continue;
            const int base = pl.rowbase[static_cast<size_t>(row_base + j * nruns + (packed >> 20))] + (packed & 0xfffff);
            for (int c = c_begin; c < c_end; ++c) {
              double v = 0.0;
              // chain of the unit that holds column c (bp_unit_col), then the products the kernel skips for it
              int qc = -1;
              for (int q = 0; q < h[H_NTILE] + ((h[H_FLAGS] & 2) ? 1 : 0) && qc < 0; ++q)
                for (int lc = 0; lc < 16; ++lc)
                  if (bp_unit_col(h[H_CT0], h[H_NTILE], q, lc) == c) { qc = q; break; }
              MHA_REQUIRE(qc >= 0, MHA_ERR_STATE, "a column of a unit belongs to none of its chains");
              const int trim = (h[H_NTILE] == 4 && !(h[H_FLAGS] & 2)) ? (h[H_FLAGS] >> 2) & 7 : 0;
              for (int s = 0; s < ks; ++s) {
                const bool second = s >= ks / 2;
                if ((trim == 1 && qc < 2 && second) || (trim == 2 && qc >= 2 && !second) || (trim == 3 && qc < 2 && !second) ||
                    (trim == 4 && qc >= 2 && second))
                  continue;
                const int bit = s * 5 + qc;
                if (!((static_cast<uint32_t>(h[H_MASK0 + bit / 32]) >> (bit % 32)) & 1u)) continue;  // a zero block of W
                for (int kk = 0; kk < 4; ++kk) {
                  const int lane = kk * 16 + row;  // A operand: row = lane & 15, k = 4 s + (lane >> 4)
                  const size_t wi = static_cast<size_t>(4 * s + kk) * stride + c;
                  v += rec[L[s * 64 + lane]] * (su * W[wi] + st * Wm[wi]);
                }
              }
              if (overwrite) vals[base + c] = fixed_class ? 0.0 : v;
              else vals[base + c] += v;
            }
          }
        }
      }
  }
}

std::vector<CopyRun> block_pattern_copy_runs(const BlockPatternPlan &pl) {
  std::vector<CopyRun> runs;
  for (int k = 0; k < pl.num_roles; ++k) {
    const int32_t *ro = &pl.role[static_cast<size_t>(k) * kBpRoleInts];
    const int64_t row_base = (static_cast<int64_t>(ro[R_ROWB_HI]) << 32) | static_cast<uint32_t>(ro[R_ROWB_LO]);
    const int nruns = ro[R_NRUNS], nblocks = ro[R_NBLOCKS];
    const int32_t *rl = &pl.runlen[static_cast<size_t>(pl.role_runlen_off[k])];
    for (int j = 1; j < nblocks; ++j)
      for (int r = 0; r < nruns; ++r)
        runs.push_back({pl.rowbase[static_cast<size_t>(row_base + r)], pl.rowbase[static_cast<size_t>(row_base + static_cast<int64_t>(j) * nruns + r)], rl[r]});
  }
  return runs;
}

BpRepPlan build_rep_plan(const BlockPatternPlan &pl) {
  MHA_REQUIRE(pl.usable, MHA_ERR_STATE, "block patterns not usable: " << pl.why);
  MHA_REQUIRE(pl.erec_elem.size() * kBpRecDoubles < (size_t(1) << 31) && pl.w.size() < (size_t(1) << 31), MHA_ERR_INVALID,
              "representatives: element records or W images beyond 32-bit offsets");
  BpRepPlan rp;
  for (int k = 0; k < pl.num_roles; ++k) {
    const int32_t *ro = &pl.role[static_cast<size_t>(k) * kBpRoleInts];
    if (ro[R_NBLOCKS] < 1) continue;
    const int64_t erec_base = (static_cast<int64_t>(ro[R_EREC_HI]) << 32) | static_cast<uint32_t>(ro[R_EREC_LO]);
    const int64_t row_base = (static_cast<int64_t>(ro[R_ROWB_HI]) << 32) | static_cast<uint32_t>(ro[R_ROWB_LO]);
    const int64_t woff = (static_cast<int64_t>(ro[R_WOFF_HI]) << 32) | static_cast<uint32_t>(ro[R_WOFF_LO]);
    const int32_t *pp = &pl.part_ptr[static_cast<size_t>(k) * (kBpWaves + 1)];
    for (int p = pp[0]; p < pp[kBpWaves]; ++p) {  // every unit of the role, whichever wavefront the full kernel gives it
      const int32_t *h = &pl.part_hdr[static_cast<size_t>(p) * kBpHdrInts];
      const int32_t *L = &pl.part_lane[static_cast<size_t>(p) * kBpLaneRows * 64];
      const bool fixed_class = h[H_FLAGS] & 1;
      const int ks = h[H_KS], len = h[H_LEN], stride = stride_for(h[H_NCT]);
      MHA_REQUIRE(fixed_class || (ks >= 1 && ks <= kBpMaxKSteps), MHA_ERR_STATE, "representatives: a unit of products with " << ks << " k-steps");
      for (int q = 0; q < h[H_NTILE] + ((h[H_FLAGS] & 2) ? 1 : 0); ++q) {
        const int32_t it[kBpRepItemInts] = {fixed_class ? 0 : ks, 4 * stride, ro[R_WDOUBLES], fixed_class ? 1 : 0};
        rp.item.insert(rp.item.end(), it, it + kBpRepItemInts);
        rp.unit.insert(rp.unit.end(), {k, p, q});
        const size_t base = rp.lane.size();
        rp.lane.resize(base + static_cast<size_t>(kBpRepLaneRows) * 64, 0);
        int32_t *R = rp.lane.data() + base;
        for (int lane = 0; lane < 64; ++lane) {
          const int col = 16 * (h[H_CT0] + q) + (lane & 15);  // plain column order: a column's products do not depend on it
          for (int s = 0; s < kBpMaxKSteps; ++s) R[s * 64 + lane] = static_cast<int32_t>(erec_base * kBpRecDoubles + L[s * 64 + lane]);
          for (int t = 0; t < 4; ++t) {
            const int packed = L[(16 + t) * 64 + lane];
            R[(16 + t) * 64 + lane] =
                packed < 0 || col >= len ? -1 : pl.rowbase[static_cast<size_t>(row_base + (packed >> 20))] + (packed & 0xfffff) + col;
          }
          R[20 * 64 + lane] = static_cast<int32_t>(woff + h[H_WOFF] + static_cast<int64_t>(lane >> 4) * stride + col);
        }
      }
    }
  }
  return rp;
}

void rep_plan_host_apply(const BlockPatternPlan &pl, const BpRepPlan &rp, const double *factors, double su, double st,
                         double *vals, int32_t *stores) {
  const int ke = pl.ke;
  auto rec = [&](int32_t r) {  // erec2 entry r, as build_erec2_kernel lays the records out
    const int e = pl.erec_elem[static_cast<size_t>(r / kBpRecDoubles)], m = r % kBpRecDoubles;
    return e >= 0 && m < ke ? factors[static_cast<size_t>(e) * ke + m] : 0.0;
  };
  for (int i = 0; i < rp.num_items(); ++i) {
    const int32_t *it = &rp.item[static_cast<size_t>(i) * kBpRepItemInts];
    const int32_t *R = &rp.lane[static_cast<size_t>(i) * kBpRepLaneRows * 64];
    const int role = rp.unit[3 * i], p = rp.unit[3 * i + 1];
    const int32_t *ro = &pl.role[static_cast<size_t>(role) * kBpRoleInts];
    const int32_t *h = &pl.part_hdr[static_cast<size_t>(p) * kBpHdrInts];
    // the W range of the part's class (stiffness half): what every load of the item must stay inside
    const int64_t wlo = ((static_cast<int64_t>(ro[R_WOFF_HI]) << 32) | static_cast<uint32_t>(ro[R_WOFF_LO])) + h[H_WOFF];
    const int64_t whi = wlo + static_cast<int64_t>(h[H_KS]) * 4 * stride_for(h[H_NCT]);
    MHA_REQUIRE(it[2] == ro[R_WDOUBLES] && whi + it[2] <= static_cast<int64_t>(pl.w.size()), MHA_ERR_STATE, "representatives: W halves misplaced");
    for (int row = 0; row < 16; ++row)
      for (int c = 0; c < 16; ++c) {
        const int lane = ((row & 3) << 4) | c;  // D register t = row >> 2 of lane (row & 3) * 16 + c
        const int dst = R[(16 + (row >> 2)) * 64 + lane];
        if (dst < 0) continue;
        double v = 0.0;
        for (int s = 0; s < it[0]; ++s)
          for (int kk = 0; kk < 4; ++kk) {
            const int a_lane = kk * 16 + row, b_lane = kk * 16 + c;  // A[row = lane & 15][k = lane >> 4], B[k][col = lane & 15]
            const int64_t wi = static_cast<int64_t>(R[20 * 64 + b_lane]) + static_cast<int64_t>(s) * it[1];
            MHA_REQUIRE(wi >= wlo && wi < whi, MHA_ERR_STATE, "representatives: a W load outside the class of its unit");
            v += rec(R[s * 64 + a_lane]) * (su * pl.w[static_cast<size_t>(wi)] + st * pl.w[static_cast<size_t>(wi + it[2])]);
          }
        vals[dst] = it[3] ? 0.0 : v;
        if (stores) ++stores[dst];
      }
  }
}

BpRepMap build_rep_map(const BlockPatternPlan &pl) {
  struct Run { int64_t crs, rep, len; };
  std::vector<Run> runs;
  BpRepMap m;
  for (int k = 0; k < pl.num_roles; ++k) {
    const int32_t *ro = &pl.role[static_cast<size_t>(k) * kBpRoleInts];
    if (ro[R_NBLOCKS] < 1) continue;
    const int64_t row_base = (static_cast<int64_t>(ro[R_ROWB_HI]) << 32) | static_cast<uint32_t>(ro[R_ROWB_LO]);
    const int32_t *rl = &pl.runlen[static_cast<size_t>(pl.role_runlen_off[k])];
    for (int r = 0; r < ro[R_NRUNS]; ++r) {
      runs.push_back({pl.rowbase[static_cast<size_t>(row_base + r)], m.size, rl[r]});
      m.size += rl[r];
    }
  }
  std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.crs < b.crs; });
  for (size_t i = 0; i < runs.size(); ++i) {
    MHA_REQUIRE(i == 0 || runs[i - 1].crs + runs[i - 1].len <= runs[i].crs, MHA_ERR_STATE, "representatives: two roles' first blocks share CRS entries");
    m.crs.push_back(runs[i].crs);
    m.rep.push_back(runs[i].rep);
    m.len.push_back(runs[i].len);
  }
  return m;
}

int64_t BpRepMap::index(int64_t e) const {
  const size_t i = static_cast<size_t>(std::upper_bound(crs.begin(), crs.end(), e) - crs.begin());
  if (i == 0 || e >= crs[i - 1] + len[i - 1]) return -1;
  return rep[i - 1] + (e - crs[i - 1]);
}

void compact_rep_plan(BpRepPlan &rp, const BpRepMap &m) {
  for (int i = 0; i < rp.num_items(); ++i) {
    int32_t *R = rp.lane.data() + static_cast<size_t>(i) * kBpRepLaneRows * 64;
    for (int t = 0; t < 4; ++t)
      for (int lane = 0; lane < 64; ++lane) {
        int32_t &d = R[(16 + t) * 64 + lane];
        if (d < 0) continue;
        const int64_t c = m.index(d);
        MHA_REQUIRE(c >= 0 && c < m.size, MHA_ERR_STATE, "representatives: an item stores outside the first blocks' rows");
        d = static_cast<int32_t>(c);
      }
  }
}

std::vector<CopyRun> block_pattern_rep_copy_runs(const BlockPatternPlan &pl, const BpRepMap &m) {
  std::vector<CopyRun> runs;
  for (int k = 0; k < pl.num_roles; ++k) {
    const int32_t *ro = &pl.role[static_cast<size_t>(k) * kBpRoleInts];
    const int64_t row_base = (static_cast<int64_t>(ro[R_ROWB_HI]) << 32) | static_cast<uint32_t>(ro[R_ROWB_LO]);
    const int nruns = ro[R_NRUNS], nblocks = ro[R_NBLOCKS];
    const int32_t *rl = &pl.runlen[static_cast<size_t>(pl.role_runlen_off[k])];
    for (int r = 0; r < nruns && nblocks > 0; ++r) {
      const int64_t src = m.index(pl.rowbase[static_cast<size_t>(row_base + r)]);
      MHA_REQUIRE(src >= 0, MHA_ERR_STATE, "representatives: a run of a first block is not in the map");
      for (int j = 0; j < nblocks; ++j)
        runs.push_back({src, pl.rowbase[static_cast<size_t>(row_base + static_cast<int64_t>(j) * nruns + r)], rl[r]});
    }
  }
  return runs;
}

}  // namespace mha
