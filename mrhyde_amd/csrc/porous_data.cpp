// porous_data.cpp -- see porous_data.hpp
#include "porous_data.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"

namespace mha {

namespace {
double chareqn(double om, double L, double eta) {
  return (eta * eta * om * om - 1.0) * std::sin(om * L) - 2.0 * eta * om * std::cos(om * L);
}
double dchareqn(double om, double L, double eta) {
  return 2.0 * om * eta * eta * std::sin(om * L) + (eta * eta * om * om - 1.0) * L * std::cos(om * L) -
         2.0 * eta * std::cos(om * L) + 2.0 * eta * om * L * std::sin(om * L);
}
}  // namespace

// reference: klexpansion::computeRoots (tools/klexpansion.hpp:38-90)
int kl_roots(int N, double L, double sigma, double eta, double *omega, double *lambda) {
  std::vector<double> roots;
  double ig = 1.0, fprev = chareqn(ig, L, eta);
  for (int iter = 0; static_cast<int>(roots.size()) < N && iter < 1000; ++iter) {
    ig += 1.0;
    double om = ig, f = chareqn(om, L, eta);
    if (f * fprev < 0) {
      fprev = f;
      for (int nl = 0; std::abs(f) > 1e-10 && nl < 10; ++nl) {
        om -= f / dchareqn(om, L, eta);
        f = chareqn(om, L, eta);
      }
      bool dup = false;
      for (double r : roots) dup = dup || std::abs(om - r) < 1e-6;
      if (!dup) roots.push_back(om);
    }
  }
  for (size_t k = 0; k < roots.size(); ++k) {
    if (omega) omega[k] = roots[k];
    if (lambda) lambda[k] = (2.0 * eta * sigma * sigma) / (eta * eta * roots[k] * roots[k] + 1.0);
  }
  return static_cast<int>(roots.size());
}

double kl_norm(double omega, double L, double eta) { return std::sqrt((eta * eta * omega * omega + 1.0) * L / 2.0 + eta); }

void kl_indices(int dim, const int *N, std::vector<int32_t> &idx) {
  MHA_REQUIRE(dim == 2 || dim == 3, MHA_ERR_INVALID, "KL indices: dim must be 2 or 3");
  for (int d = 0; d < dim; ++d) MHA_REQUIRE(N[d] >= 1, MHA_ERR_INVALID, "KL indices: N must be positive");
  const int nz = dim == 3 ? N[2] : 1, amax = N[0] + N[1] + nz - 2;
  idx.clear();
  for (int a = 0; a <= amax; ++a)
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < N[1]; ++j)
        for (int i = 0; i < N[0]; ++i)
          if (i + j + k == a) {
            idx.push_back(i);
            idx.push_back(j);
            if (dim == 3) idx.push_back(k);
          }
}

// reference: Data::findClosestPoint (tools/data.cpp:391-420) -- the brute-force variant's metric and tie rule
void closest_points(int dim, int64_t nq, const double *query, int64_t np, const double *points, int32_t *idx) {
  MHA_REQUIRE(dim >= 1 && dim <= 3, MHA_ERR_INVALID, "closest points: dim must be 1, 2 or 3");
  MHA_REQUIRE(np >= 1 && np < (int64_t(1) << 31), MHA_ERR_INVALID, "closest points: need 1 .. 2^31-1 data points");
  MHA_REQUIRE(nq >= 0 && (nq == 0 || (query && idx)) && points, MHA_ERR_INVALID, "closest points: null argument");
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, h[3] = {1, 1, 1};
  for (int d = 0; d < dim; ++d) { lo[d] = std::numeric_limits<double>::infinity(); hi[d] = -lo[d]; }
  for (int64_t p = 0; p < np; ++p)
    for (int d = 0; d < dim; ++d) {
      const double x = points[p * dim + d];
      MHA_REQUIRE(std::isfinite(x), MHA_ERR_INVALID, "closest points: non-finite data point " << p);
      lo[d] = std::min(lo[d], x);
      hi[d] = std::max(hi[d], x);
    }
  // about one point per bucket along the directions the points span
  int spanned = 0;
  for (int d = 0; d < dim; ++d) spanned += hi[d] > lo[d];
  const int per = spanned ? std::max(1, static_cast<int>(std::pow(static_cast<double>(np), 1.0 / spanned))) : 1;
  int g[3] = {1, 1, 1};
  double ext = 0.0;
  for (int d = 0; d < dim; ++d) {
    if (hi[d] > lo[d]) { g[d] = std::min(per, 1 << 12); h[d] = (hi[d] - lo[d]) / g[d]; }
    ext = std::max(ext, hi[d] - lo[d]);
  }
  auto cell = [&](int d, double x) {
    const double c = std::floor((x - lo[d]) / h[d]);
    return c < 0 ? 0 : c >= g[d] ? g[d] - 1 : static_cast<int>(c);
  };
  const int64_t ncell = static_cast<int64_t>(g[0]) * g[1] * g[2];
  std::vector<int64_t> start(ncell + 1, 0);
  std::vector<int32_t> order(np);
  std::vector<int64_t> key(np);
  for (int64_t p = 0; p < np; ++p) {
    int64_t k = 0;
    for (int d = dim - 1; d >= 0; --d) k = k * g[d] + cell(d, points[p * dim + d]);
    key[p] = k;
    ++start[k + 1];
  }
  for (int64_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t p = 0; p < np; ++p) order[fill[key[p]]++] = static_cast<int32_t>(p);  // ascending index per bucket
  }
  // (a point whose bucket was rounded across a boundary lies within round-off of it: the stopping test keeps a margin)
  const double margin = 1e-9 * (ext > 0 ? ext : 1.0);
  for (int64_t q = 0; q < nq; ++q) {
    const double *x = query + q * dim;
    int c[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) c[d] = cell(d, x[d]);
    double best = std::numeric_limits<double>::infinity();
    int32_t bi = -1;
    auto visit = [&](const int *cc) {
      int64_t k = 0;
      for (int d = dim - 1; d >= 0; --d) k = k * g[d] + cc[d];
      for (int64_t s = start[k]; s < start[k + 1]; ++s) {
        const int32_t p = order[s];
        double t = 0.0;
        for (int d = 0; d < dim; ++d) {
          const double df = points[static_cast<int64_t>(p) * dim + d] - x[d];
          t += df * df;
        }
        if (t < best || (t == best && p < bi)) { best = t; bi = p; }
      }
    };
    for (int r = 0;; ++r) {
      // the buckets at Chebyshev distance r from c
      int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
      for (int d = 0; d < 3; ++d) { a[d] = d < dim ? std::max(0, c[d] - r) : 0; b[d] = d < dim ? std::min(g[d] - 1, c[d] + r) : 0; }
      int cc[3];
      for (cc[2] = a[2]; cc[2] <= b[2]; ++cc[2])
        for (cc[1] = a[1]; cc[1] <= b[1]; ++cc[1])
          for (cc[0] = a[0]; cc[0] <= b[0]; ++cc[0]) {
            bool ring = false;
            for (int d = 0; d < dim; ++d) ring = ring || cc[d] == c[d] - r || cc[d] == c[d] + r;
            if (ring) visit(cc);
          }
      // every point outside the searched box lies beyond one of its faces that is not the grid's edge
      double lb = std::numeric_limits<double>::infinity();
      for (int d = 0; d < dim; ++d) {
        if (c[d] - r > 0) lb = std::min(lb, x[d] - (lo[d] + (c[d] - r) * h[d]));
        if (c[d] + r < g[d] - 1) lb = std::min(lb, (lo[d] + (c[d] + r + 1) * h[d]) - x[d]);
      }
      if (std::isinf(lb)) break;  // the whole grid has been searched
      lb -= margin;
      if (bi >= 0 && lb > 0 && lb * lb > best) break;
    }
    idx[q] = bi;
  }
}

}  // namespace mha
