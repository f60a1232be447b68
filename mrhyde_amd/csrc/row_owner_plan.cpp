#include "row_owner_plan.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <utility>

namespace mha {

std::vector<double> affine_reference_tables(const RefTables &ref, const int32_t *offs, int dim, int n, int nq) {
  const int nsym = dim * (dim + 1) / 2;
  std::vector<double> khat(static_cast<size_t>(nsym + 1) * n * n, 0.0);
  for (int ib = 0; ib < n; ++ib)
    for (int jb = 0; jb < n; ++jb) {
      const size_t idx = static_cast<size_t>(offs[ib]) * n + offs[jb];
      int k = 0;
      for (int a = 0; a < dim; ++a)
        for (int c = a; c < dim; ++c, ++k) {
          double s = 0.0;
          for (int q = 0; q < nq; ++q) {
            const double *gi = &ref.grad[(static_cast<size_t>(ib) * nq + q) * dim];
            const double *gj = &ref.grad[(static_cast<size_t>(jb) * nq + q) * dim];
            s += ref.wts[q] * (a == c ? gi[a] * gj[a] : gi[a] * gj[c] + gi[c] * gj[a]);
          }
          khat[static_cast<size_t>(k) * n * n + idx] = s;
        }
      double m = 0.0;
      for (int q = 0; q < nq; ++q) m += ref.wts[q] * ref.basis[ib * nq + q] * ref.basis[jb * nq + q];
      khat[static_cast<size_t>(nsym) * n * n + idx] = m;
    }
  return khat;
}

AffineTables1D collocation_derivative(const RefTables &ref, int order) {
  const int m = order + 1;
  AffineTables1D t;
  for (int i = 0; i < m * m; ++i) t.phi[i] = ref.phi1d[i];
  for (int q = 0; q < m; ++q) { t.gw[q] = ref.gauss_wts[q]; t.gp[q] = ref.gauss_pts[q]; }
  // inv = Phi^-1 with Phi[i][q] = phi_i(xi_q)
  std::vector<double> a(ref.phi1d.begin(), ref.phi1d.begin() + m * m), inv(m * m, 0.0);
  for (int i = 0; i < m; ++i) inv[i * m + i] = 1.0;
  for (int c = 0; c < m; ++c) {
    int piv = c;
    for (int r = c + 1; r < m; ++r)
      if (std::fabs(a[r * m + c]) > std::fabs(a[piv * m + c])) piv = r;
    for (int k = 0; k < m; ++k) { std::swap(a[c * m + k], a[piv * m + k]); std::swap(inv[c * m + k], inv[piv * m + k]); }
    const double d = 1.0 / a[c * m + c];
    for (int k = 0; k < m; ++k) { a[c * m + k] *= d; inv[c * m + k] *= d; }
    for (int r = 0; r < m; ++r) {
      if (r == c) continue;
      const double f = a[r * m + c];
      for (int k = 0; k < m; ++k) { a[r * m + k] -= f * a[c * m + k]; inv[r * m + k] -= f * inv[c * m + k]; }
    }
  }
  for (int q = 0; q < m; ++q)
    for (int qp = 0; qp < m; ++qp) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += ref.dphi1d[i * m + q] * inv[qp * m + i];
      t.dcol[q * m + qp] = s;
    }
  return t;
}

std::vector<int> pair_lid_slots(const std::vector<int32_t> &emask, int n) {
  std::vector<double> both(static_cast<size_t>(n) * n, 0.0), cnt(n, 0.0);
  const size_t stride = std::max<size_t>(1, emask.size() / 200000);  // a sample is plenty
  for (size_t i = 0; i < emask.size(); i += stride) {
    const uint32_t m = static_cast<uint32_t>(emask[i]);
    for (int a = 0; a < n && a < 32; ++a) {
      if (!((m >> a) & 1u)) continue;
      cnt[a] += 1.0;
      for (int c = a + 1; c < n && c < 32; ++c)
        if ((m >> c) & 1u) both[static_cast<size_t>(a) * n + c] += 1.0;
    }
  }
  std::vector<int> pairs(2 * ((n + 1) / 2), -1);
  std::vector<char> used(n, 0);
  for (int r = 0; r < n / 2; ++r) {
    int ba = -1, bc = -1;
    double best = -1.0;
    for (int a = 0; a < n; ++a)
      for (int c = a + 1; c < n; ++c) {
        if (used[a] || used[c]) continue;
        const double uni = cnt[a] + cnt[c] - both[static_cast<size_t>(a) * n + c];
        const double jac = uni > 0.0 ? both[static_cast<size_t>(a) * n + c] / uni : 0.0;
        if (jac > best) { best = jac; ba = a; bc = c; }
      }
    pairs[2 * r] = ba;
    pairs[2 * r + 1] = bc;
    used[ba] = used[bc] = 1;
  }
  if (n % 2)
    for (int a = 0; a < n; ++a)
      if (!used[a]) pairs[2 * (n / 2)] = a;
  return pairs;
}

K1Plan build_k1_plan(int nelem, int n, int dim, const int32_t *lids, const int32_t *offs, const double *geo,
                     K1Order forced, int row_budget) {
  constexpr int T = kK1PlanThreads;
  K1Plan p;
  p.axis_aligned = true;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int e = 0; e < nelem; ++e) {
    const double *g = &geo[static_cast<size_t>(e) * kGeoRec];
    for (int r = 0; r < dim; ++r) {
      lo[r] = std::min(lo[r], g[kGeoXc + r]);
      hi[r] = std::max(hi[r], g[kGeoXc + r]);
      for (int c = 0; c < dim; ++c)
        if (r != c && g[kGeoJ + r * dim + c] != 0.0) p.axis_aligned = false;
    }
  }
  const int G = (nelem + T - 1) / T;
  std::vector<int32_t> &wg_elems = p.wg_elems, &rp = p.row_ptr, &rows = p.rows, tmp;
  std::vector<uint16_t> &loc = p.loc;
  wg_elems.resize(static_cast<size_t>(G) * T);
  int max_rows = 0;
  auto build = [&](bool natural) {
    std::vector<std::pair<uint64_t, int32_t>> keyed(nelem);
    for (int e = 0; e < nelem; ++e) {
      uint64_t key = 0;
      if (!natural) {
        uint32_t q[3] = {0, 0, 0};
        for (int r = 0; r < dim; ++r) {
          const double w = hi[r] > lo[r] ? (geo[static_cast<size_t>(e) * kGeoRec + kGeoXc + r] - lo[r]) / (hi[r] - lo[r]) : 0.0;
          q[r] = static_cast<uint32_t>(std::min(1048575.0, std::max(0.0, w * 1048575.0)));
        }
        for (int bit = 19; bit >= 0; --bit)
          for (int r = dim - 1; r >= 0; --r) key = (key << 1) | ((q[r] >> bit) & 1u);
      }
      keyed[e] = {key, e};
    }
    std::sort(keyed.begin(), keyed.end());
    for (size_t i = 0; i < wg_elems.size(); ++i) wg_elems[i] = keyed[std::min<size_t>(i, nelem - 1)].second;
    rp.assign(static_cast<size_t>(G) + 1, 0);
    rows.clear();
    rows.reserve(static_cast<size_t>(nelem) * n / 2);
    loc.assign(static_cast<size_t>(G) * n * T, 0);
    max_rows = 0;
    for (int g = 0; g < G; ++g) {
      const int cnt = std::min(T, nelem - g * T);
      tmp.clear();
      for (int t = 0; t < cnt; ++t) {
        const int32_t *L = &lids[static_cast<size_t>(wg_elems[static_cast<size_t>(g) * T + t]) * n];
        tmp.insert(tmp.end(), L, L + n);
      }
      std::sort(tmp.begin(), tmp.end());
      tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
      for (int t = 0; t < cnt; ++t) {
        const int32_t *L = &lids[static_cast<size_t>(wg_elems[static_cast<size_t>(g) * T + t]) * n];
        for (int ib = 0; ib < n; ++ib)
          loc[(static_cast<size_t>(g) * n + ib) * T + t] =
              static_cast<uint16_t>(std::lower_bound(tmp.begin(), tmp.end(), L[offs[ib]]) - tmp.begin());
      }
      rows.insert(rows.end(), tmp.begin(), tmp.end());
      rp[g + 1] = static_cast<int32_t>(rows.size());
      max_rows = std::max(max_rows, static_cast<int>(tmp.size()));
    }
    p.morton = !natural;
  };
  build(forced != K1Order::morton);
  if (forced == K1Order::automatic && max_rows > row_budget) {
    const int natural_rows = max_rows;
    build(false);
    if (max_rows >= natural_rows) build(true);
  }
  p.max_rows = (max_rows + 1) / 2 * 2;
  return p;
}

ShapeTable distinct_shapes(const double *geo, int nelem, int dim) {
  static_assert(kGeoXc == 16, "the shape part of a geometry record is its first 16 doubles");
  std::unordered_map<std::string, int32_t> seen;
  ShapeTable st;
  st.index.resize(nelem);
  const int nsym = dim * (dim + 1) / 2;
  for (int e = 0; e < nelem; ++e) {
    double rec[16];
    for (int k = 0; k < 16; ++k) {  // (entries a 2-D record does not use are not part of the shape)
      const bool used = k < nsym || k == kGeoDet || (k >= kGeoJ && k < kGeoJ + dim * dim);
      rec[k] = used ? geo[static_cast<size_t>(e) * kGeoRec + k] : 0.0;
    }
    auto it = seen.emplace(std::string(reinterpret_cast<const char *>(rec), sizeof(rec)), static_cast<int32_t>(seen.size()));
    if (it.second) st.shapes.insert(st.shapes.end(), rec, rec + 16);
    st.index[e] = it.first->second;
  }
  st.count = static_cast<int>(seen.size());
  return st;
}

}  // namespace mha
