#include "porous_plan.hpp"

#include <algorithm>
#include <cstring>
#include <unordered_map>

namespace mha {

PorousDirectPlan porous_direct_plan(int nrows, int nelem, int n, const int32_t *lids, const int32_t *offs,
                                    const int32_t *rowptr, const int32_t *colind, const RowIncidence &inc) {
  PorousDirectPlan p;
  const std::vector<int32_t> &ptr = inc.ptr, &elem = inc.elem, &lpos = inc.lpos;
  for (int r = 0; r < nrows; ++r) {
    const int ni = ptr[r + 1] - ptr[r];
    if (ni > 2) { p.why = "a row with more than two incident elements"; return p; }
    if (ni == 2) {
      const int32_t *a = &lids[static_cast<size_t>(elem[ptr[r]]) * n], *b = &lids[static_cast<size_t>(elem[ptr[r] + 1]) * n];
      int shared = 0;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) shared += a[i] == b[j];
      if (shared != 1) { p.why = "two elements share more than one dof"; return p; }
    }
  }
  for (int e = 0; e < nelem; ++e)  // (an element listing a dof twice would add twice into one entry)
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j)
        if (lids[static_cast<size_t>(e) * n + i] == lids[static_cast<size_t>(e) * n + j]) { p.why = "repeated dof in an element"; return p; }
  // which incidence of its row an element is (dof order), and where the diagonal of a face row sits in the CRS
  std::vector<int32_t> p2d(n, 0);
  for (int f = 0; f < n; ++f) p2d[offs[f]] = f;
  p.side.assign(static_cast<size_t>(nelem) * n, 0);
  p.diag.assign(nrows, -1);
  for (int r = 0; r < nrows; ++r) {
    bool face = false;
    for (int k = ptr[r]; k < ptr[r + 1]; ++k) {
      const int d = p2d[lpos[k]];
      p.side[static_cast<size_t>(elem[k]) * n + d] = static_cast<uint8_t>(k - ptr[r]);
      face = face || d > 0;
    }
    if (face)
      for (int k = rowptr[r]; k < rowptr[r + 1]; ++k)
        if (colind[k] == r) p.diag[r] = k;
  }
  p.usable = true;
  return p;
}

PorousDatabasePlan porous_database_plan(int nrows, int nelem, int n, int nn, int d, const int32_t *offs,
                                        const int32_t *rowptr, const int32_t *colind, const double *nodes,
                                        const int8_t *orient, const uint8_t *fixed, const uint8_t *slot,
                                        const RowIncidence &inc) {
  PorousDatabasePlan p;
  for (int e = 1; e < nelem; ++e)
    for (int k = 1; k < nn; ++k)
      for (int c = 0; c < d; ++c) {
        const double a = nodes[(static_cast<size_t>(e) * nn + k) * d + c] - nodes[static_cast<size_t>(e) * nn * d + c];
        const double b0 = nodes[static_cast<size_t>(k) * d + c] - nodes[c];
        if (std::memcmp(&a, &b0, sizeof(double)) != 0) { p.why = "elements of different shapes"; return p; }
      }
  if (orient)
    for (int e = 1; e < nelem; ++e)
      if (std::memcmp(&orient[static_cast<size_t>(e) * n], &orient[0], n) != 0) { p.why = "orientation signs differ between elements"; return p; }
  {  // is the common shape an axis-aligned box?  (shards vertex order: bit pattern of vertex k = (k in {1,2,5,6}, k in {2,3,6,7}, k >= 4))
    p.axis_aligned = true;
    for (int k = 0; k < nn; ++k) {
      const bool bit[3] = {k == 1 || k == 2 || k == 5 || k == 6, k == 2 || k == 3 || k == 6 || k == 7, k >= 4};
      const int ref[3] = {1, 3, 4};  // the vertices one step from vertex 0 in x, y, z
      for (int c = 0; c < d; ++c) {
        const double rel = nodes[static_cast<size_t>(k) * d + c] - nodes[c];
        const double want = bit[c] ? nodes[static_cast<size_t>(ref[c]) * d + c] - nodes[c] : 0.0;
        if (rel != want) p.axis_aligned = false;
      }
    }
  }
  // ---- row classes ----
  const std::vector<int32_t> &ptr = inc.ptr, &elem = inc.elem, &lpos = inc.lpos;
  std::vector<int32_t> p2d(n, 0);
  for (int f = 0; f < n; ++f) p2d[offs[f]] = f;
  std::unordered_map<std::string, int32_t> classes;
  std::vector<int32_t> cls(nrows, -1);
  std::string key;
  for (int r = 0; r < nrows; ++r) {
    if (fixed && fixed[r]) continue;  // fixed rows: computed (zeroed) by the finishing pass
    key.clear();
    key.push_back(static_cast<char>(rowptr[r + 1] - rowptr[r]));
    for (int k = ptr[r]; k < ptr[r + 1]; ++k) {
      key.push_back(static_cast<char>(p2d[lpos[k]]));
      const uint8_t *srow = &slot[(static_cast<size_t>(elem[k]) * n + lpos[k]) * n];
      for (int f = 0; f < n; ++f) key.push_back(static_cast<char>(srow[offs[f]]));
    }
    cls[r] = classes.emplace(key, static_cast<int32_t>(classes.size())).first->second;
  }
  const int nc = static_cast<int>(classes.size());
  std::vector<int32_t> rep_entry(nc, -1), len_of(nc, 0), K_of(nc, 0);
  std::vector<uint8_t> replicated(nrows, 0);
  // pass 1: representatives = the first K rows of the first long run of a class
  for (int r = 0; r < nrows;) {
    int r1 = r + 1;
    while (r1 < nrows && cls[r1] == cls[r]) ++r1;
    const int c = cls[r];
    if (c >= 0 && rep_entry[c] < 0) {
      const int len = rowptr[r + 1] - rowptr[r];
      const int K = len > 0 ? (128 + len - 1) / len + 2 : 0;
      if (len > 0 && r1 - r >= 2 * K) { rep_entry[c] = rowptr[r]; len_of[c] = len; K_of[c] = K; for (int q = r + K; q < r1; ++q) replicated[q] = 1; }
    }
    r = r1;
  }
  // pass 2: every other row of a class that has representatives
  for (int r = 0; r < nrows; ++r) {
    const int c = cls[r];
    if (c < 0 || rep_entry[c] < 0 || replicated[r]) continue;
    const bool is_rep = rowptr[r] >= rep_entry[c] && rowptr[r] < rep_entry[c] + K_of[c] * len_of[c];
    if (!is_rep) replicated[r] = 1;
  }
  // copy runs of the replicated ranges (maximal runs of replicated rows of one class): the class's K representative
  // rows repeat with period len, so every K * len entries of a range read the representatives from their first entry
  for (int r = 0; r < nrows;) {
    if (!replicated[r]) { ++p.computed_rows; ++r; continue; }
    int r1 = r + 1;
    while (r1 < nrows && replicated[r1] && cls[r1] == cls[r]) ++r1;
    const int c = cls[r];
    const int64_t dbeg = rowptr[r], dend = rowptr[r1], period = static_cast<int64_t>(K_of[c]) * len_of[c];
    for (int64_t d0 = dbeg; d0 < dend; d0 += period) p.runs.push_back({rep_entry[c], d0, std::min(period, dend - d0)});
    r = r1;
  }
  if (p.runs.empty()) { p.why = "no class has a run long enough to replicate"; return p; }
  // elements incident to computed rows store their entries; diagonal positions of the computed face rows only
  p.jacflag.assign(nelem, 0);
  p.diag.assign(nrows, -1);
  for (int r = 0; r < nrows; ++r) {
    if (replicated[r]) continue;
    bool face = false;
    for (int k = ptr[r]; k < ptr[r + 1]; ++k) { p.jacflag[elem[k]] = 1; face = face || p2d[lpos[k]] > 0; }
    if (face)
      for (int k = rowptr[r]; k < rowptr[r + 1]; ++k)
        if (colind[k] == r) p.diag[r] = k;
  }
  for (int e = 0; e < nelem; ++e)
    if (p.jacflag[e]) p.elist.push_back(e);
  p.num_classes = nc;
  p.usable = true;
  return p;
}

}  // namespace mha
