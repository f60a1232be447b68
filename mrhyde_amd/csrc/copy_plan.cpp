// copy_plan.cpp -- see copy_plan.hpp.
#include "copy_plan.hpp"

#include <algorithm>
#include <climits>

#include "common.hpp"

namespace mha {

namespace {

void push_segment(CopyPlan &p, int64_t dst, int64_t off) {
  const int n = p.num_segs();
  if (n > 0 && p.seg[2 * n - 1] == off) return;  // neighbours with the same offset: one segment
  p.seg.push_back(static_cast<int32_t>(dst));
  p.seg.push_back(static_cast<int32_t>(off));
}

// work items (in place: spans holding at least one entry of a non-zero offset; separate source: every span) + sentinels
void finish_plan(CopyPlan &p) {
  const int64_t nnz = p.nnz;
  const int ns = p.num_segs();
  int s = 0;
  for (int64_t b = 0; b < nnz; b += kCopySpanEntries) {
    const int64_t e = std::min<int64_t>(b + kCopySpanEntries, nnz);
    while (s + 1 < ns && p.seg[2 * (s + 1)] <= b) ++s;
    int t = s;
    bool copies = p.nsrc > 0 || p.seg[2 * s + 1] != 0;
    while (t + 1 < ns && p.seg[2 * (t + 1)] < e) {
      ++t;
      copies = copies || p.seg[2 * t + 1] != 0;
    }
    if (!copies) continue;
    p.item.push_back(static_cast<int32_t>(b / kCopyLineEntries));
    p.item.push_back(s);
    p.item.push_back(t - s + 1);
    p.item.push_back(0);
    p.max_item_segs = std::max(p.max_item_segs, t - s + 1);
  }
  // sentinels: the kernel reads kCopySegRegs records from an item's first without a bound; past the list they start
  // after every entry and match none
  for (int k = 0; k < kCopySegRegs; ++k) {
    p.seg.push_back(INT32_MAX);
    p.seg.push_back(0);
  }
}

}  // namespace

CopyPlan build_copy_plan(std::vector<CopyRun> runs, int64_t nnz) {
  MHA_REQUIRE(nnz >= 0 && nnz <= INT32_MAX - 2 * kCopySpanEntries, MHA_ERR_INVALID, "copy plan: " << nnz << " entries do not fit 32-bit offsets");
  runs.erase(std::remove_if(runs.begin(), runs.end(), [](const CopyRun &r) { return r.len <= 0 || r.src == r.dst; }), runs.end());
  std::sort(runs.begin(), runs.end(), [](const CopyRun &a, const CopyRun &b) { return a.dst < b.dst; });
  for (size_t i = 0; i < runs.size(); ++i) {
    const CopyRun &r = runs[i];
    MHA_REQUIRE(r.dst >= 0 && r.src >= 0 && r.dst + r.len <= nnz && r.src + r.len <= nnz, MHA_ERR_INVALID, "copy plan: run outside [0, " << nnz << ")");
    MHA_REQUIRE(i == 0 || runs[i - 1].dst + runs[i - 1].len <= r.dst, MHA_ERR_INVALID, "copy plan: destinations overlap at entry " << r.dst);
  }
  for (const CopyRun &r : runs) {  // a source never reads a copied entry: the first destination interval ending past src
    auto it = std::upper_bound(runs.begin(), runs.end(), r.src, [](int64_t s, const CopyRun &q) { return s < q.dst + q.len; });
    MHA_REQUIRE(it == runs.end() || it->dst >= r.src + r.len, MHA_ERR_INVALID, "copy plan: run reads copied entries at " << r.src);
  }
  CopyPlan p;
  p.nnz = nnz;
  auto push = [&](int64_t dst, int64_t off) { push_segment(p, dst, off); };
  int64_t pos = 0;
  for (const CopyRun &r : runs) {
    if (r.dst > pos) push(pos, 0);
    push(r.dst, r.src - r.dst);
    pos = r.dst + r.len;
    p.copied += r.len;
  }
  if (pos < nnz || p.seg.empty()) push(pos, 0);
  finish_plan(p);
  return p;
}

CopyPlan build_copy_plan_from(std::vector<CopyRun> runs, int64_t nnz, int64_t nsrc) {
  MHA_REQUIRE(nnz > 0 && nnz <= INT32_MAX - 2 * kCopySpanEntries && nsrc > 0 && nsrc <= nnz, MHA_ERR_INVALID,
              "copy plan: " << nnz << " entries from " << nsrc << " do not fit 32-bit offsets");
  runs.erase(std::remove_if(runs.begin(), runs.end(), [](const CopyRun &r) { return r.len <= 0; }), runs.end());
  std::sort(runs.begin(), runs.end(), [](const CopyRun &a, const CopyRun &b) { return a.dst < b.dst; });
  CopyPlan p;
  p.nnz = nnz;
  p.nsrc = nsrc;
  int64_t pos = 0;
  for (const CopyRun &r : runs) {
    MHA_REQUIRE(r.src >= 0 && r.src + r.len <= nsrc, MHA_ERR_INVALID, "copy plan: run reads outside the source's [0, " << nsrc << ")");
    MHA_REQUIRE(r.dst == pos, MHA_ERR_INVALID, "copy plan: the runs do not tile the destination at entry " << pos);
    push_segment(p, r.dst, r.src - r.dst);
    pos = r.dst + r.len;
    p.copied += r.len;
  }
  MHA_REQUIRE(pos == nnz, MHA_ERR_INVALID, "copy plan: the runs end at entry " << pos << " of " << nnz);
  finish_plan(p);
  return p;
}

void copy_plan_host_apply(const CopyPlan &plan, double *vals, int32_t *stores, const double *src) {
  const int64_t nnz = plan.nnz;
  MHA_REQUIRE((src != nullptr) == (plan.nsrc > 0), MHA_ERR_INVALID, "copy plan: a separate-source plan and only that takes a source buffer");
  constexpr int U = kCopySpanEntries / kCopyWaveEntries;
  std::vector<double> x(kCopySpanEntries);
  std::vector<uint8_t> ok(kCopySpanEntries);
  for (int it = 0; it < plan.num_items(); ++it) {
    const int32_t *w = &plan.item[4 * static_cast<size_t>(it)];
    const int64_t s0 = static_cast<int64_t>(w[0]) * kCopyLineEntries;
    const int first = w[1], nseg = w[2];
    for (int u = 0; u < U; ++u)
      for (int lane = 0; lane < 64; ++lane)
        for (int h = 0; h < 2; ++h) {
          const int64_t e = s0 + u * kCopyWaveEntries + 2 * lane + h;
          int off = 0;
          for (int j = 0; j < nseg; j += kCopySegRegs)  // the kernel's register groups of segment records
            for (int k = 0; k < kCopySegRegs; ++k) {
              const size_t q = static_cast<size_t>(first + j + k);
              if (e >= plan.seg[2 * q]) off = plan.seg[2 * q + 1];
            }
          const int i = u * kCopyWaveEntries + 2 * lane + h;
          ok[i] = e < nnz;
          const int64_t from = ok[i] ? e + off : 0;
          MHA_REQUIRE(!src || (from >= 0 && from < plan.nsrc), MHA_ERR_STATE, "copy plan: entry " << e << " loads outside the source");
          x[i] = src ? src[from] : vals[from];
        }
    for (int i = 0; i < kCopySpanEntries; ++i)
      if (ok[i]) {
        vals[s0 + i] = x[i];
        if (stores) ++stores[s0 + i];
      }
  }
}

}  // namespace mha
