// porous_plan.hpp -- host-side plans of the porousMixed direct form and its database mode (kernels/porous_element.hip;
// AssemblyManager::porousDirectUsable / porousDatabaseUsable upload them): pure functions of host arrays.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "copy_plan.hpp"
#include "mesh.hpp"

namespace mha {

// The direct form rests on one property of the mesh: any two elements share at most ONE dof (a face), so that a matrix
// entry (i, j), i != j, has one contributing element and a row at most two.  Checked on the LID lists; !usable: why.
struct PorousDirectPlan {
  bool usable = false;
  std::string why;
  std::vector<uint8_t> side;  // [E][n] (dof order): which incidence of its row the element is
  std::vector<int32_t> diag;  // [nrows] CRS position of the diagonal of a face row, -1 otherwise
};
PorousDirectPlan porous_direct_plan(int nrows, int nelem, int n, const int32_t *lids, const int32_t *offsets,
                                    const int32_t *rowptr, const int32_t *colind, const RowIncidence &inc);

// Database mode of the direct form.  Preconditions: every element has the same vertex offsets from its first vertex and
// the same orientation signs, bit for bit (then the direct kernel, which works on relative coordinates, produces the same
// matrix for every element).  Rows are classified by what determines their values: fixed flag, and per incident element
// its local dof and the slots of the element's columns in the row.  Per class the first run of >= 2 K consecutive rows
// gives K = ceil(128 / len) + 2 representative rows (enough for any 1 KB chunk to be sourced contiguously from their
// periodic image); every other row of a class that has representatives is REPLICATED; the rest (fixed rows, short or
// rare classes, the representatives) are COMPUTED as before, by the elements incident to them.
struct PorousDatabasePlan {
  bool usable = false;
  std::string why;
  bool axis_aligned = false;     // the common element shape is an axis-aligned box
  std::vector<uint8_t> jacflag;  // [E]: the element is incident to a computed row and stores its entries
  std::vector<int32_t> elist;    // the elements with jacflag set
  std::vector<int32_t> diag;     // [nrows] diagonal positions of the COMPUTED face rows, -1 otherwise
  std::vector<CopyRun> runs;     // the replicated rows' entries from the representatives' (copy_plan.hpp)
  int num_classes = 0;
  int64_t computed_rows = 0;
};
// nodes [E][nnodes][dim]; orient [E][n] or null; fixed [nrows] or null; slot [E][n][n]: the element-major one-byte CRS
// slot map (position of column LIDs[e][j] inside row LIDs[e][i], LID-position order)
PorousDatabasePlan porous_database_plan(int nrows, int nelem, int n, int nnodes, int dim, const int32_t *offsets,
                                        const int32_t *rowptr, const int32_t *colind, const double *nodes,
                                        const int8_t *orient, const uint8_t *fixed, const uint8_t *slot,
                                        const RowIncidence &inc);

}  // namespace mha
