// porous_data.hpp -- host-side tools of porousMixed's heterogeneous permeability: the 1-D Karhunen-Loeve expansions, the
// total order of their multi-indices, and the exact nearest-point search behind mesh-data import.
#pragma once
#include <cstdint>
#include <vector>

namespace mha {

// One 1-D KL expansion (reference: tools/klexpansion.hpp): the first N roots omega of
//   (eta^2 w^2 - 1) sin(w L) - 2 eta w cos(w L),
// scanned from w = 1 in steps of 1 with at most 10 Newton steps each (|f| < 1e-10), a root within 1e-6 of an earlier
// one dropped, at most 1000 steps; lambda = 2 eta sigma^2 / (eta^2 w^2 + 1).  Returns the number of roots found (<= N).
int kl_roots(int N, double L, double sigma, double eta, double *omega, double *lambda);

// phi(x) = (eta w cos w x + sin w x) / norm, norm = sqrt((eta^2 w^2 + 1) L / 2 + eta)
double kl_norm(double omega, double L, double eta);

// The multi-indices of a dim-D expansion with N[d] terms per direction in total order (porousMixed.cpp:73-118): by
// alpha = i + j (+ k), then z, then y, then x.  idx: [prod N][dim].
void kl_indices(int dim, const int *N, std::vector<int32_t> &idx);

// For every query point the index of the nearest of np points (squared Euclidean distance summed in coordinate order;
// ties to the lowest index): exact, through a uniform grid of buckets searched ring by ring.
void closest_points(int dim, int64_t nq, const double *query, int64_t np, const double *points, int32_t *idx);

}  // namespace mha
