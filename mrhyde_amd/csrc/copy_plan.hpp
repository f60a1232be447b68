// copy_plan.hpp -- the line-aligned copy plan of the database modes (kernels/line_copy.hip).
//
// Both database modes (thermal geometry database: AssemblyManager::prepareBlockPattern; porousMixed row classes:
// porous_plan.hpp) compute a few representative CRS entries and copy them into the rest of the
// value array.  The caller describes the copy as RUNS (source entry, destination entry, length) inside vals[0, nnz);
// every entry no run covers is IN PLACE: written earlier on the same stream, left as it is.
//
// The plan cuts the DESTINATION into aligned spans of kCopySpanLines 128-byte lines and gives every span that holds a
// copied entry to one wavefront, which stores each of its lines whole, once (16 bytes per lane, one line per 8 lanes).
// A lane finds its source through the SEGMENTS: a destination-sorted list that tiles [0, nnz) without gaps,
// {first entry, source - destination}, in-place stretches with offset 0, neighbours with equal offsets merged.  In-place
// lanes of a kept span read back their own entry and store the same bits.  Entries at or past nnz are never stored.
//
// A plan with a SEPARATE SOURCE (build_copy_plan_from; the thermal geometry database, whose representatives live in a
// compact buffer of their own that is kept from one assembly to the next) has no in-place entries: its runs tile
// [0, nnz), a segment's offset is (entry of the source buffer) - (destination entry), offset 0 is an offset like any
// other, and every span is a work item.  The caller's array is written only.
#pragma once
#include <cstdint>
#include <vector>

namespace mha {

constexpr int kCopyLineEntries = 16;                     // doubles per 128-byte line
constexpr int kCopyWaveEntries = 128;                    // one 16-byte store instruction of a wavefront: 8 lines
constexpr int kCopySpanLines = 32;                       // lines of a work item, a multiple of 8 (profiles/database_copy.md)
constexpr int kCopySpanEntries = kCopySpanLines * kCopyLineEntries;
constexpr int kCopySegRegs = 8;                          // segment records a wavefront holds at once (more: a loop)

struct CopyRun {
  int64_t src, dst, len;
};

struct CopyPlan {
  int64_t nnz = 0;
  int64_t nsrc = 0;           // entries of the separate source buffer; 0: the plan copies inside vals
  std::vector<int32_t> seg;   // [num_segs][2]: first destination entry, source - destination; the last
                              // kCopySegRegs records are sentinels {INT32_MAX, 0}
  std::vector<int32_t> item;  // [num_items][4]: first line of the span, its first segment, segments it meets, 0
  int num_segs() const { return static_cast<int>(seg.size() / 2); }
  int num_items() const { return static_cast<int>(item.size() / 4); }
  int64_t copied = 0;         // entries covered by runs
  int max_item_segs = 0;      // diagnostics
};

// runs: any order; they must lie inside [0, nnz), not overlap one another as destinations, and read only in-place
// entries (a run's source is never another run's destination).  Throws MHA_ERR_INVALID otherwise.
CopyPlan build_copy_plan(std::vector<CopyRun> runs, int64_t nnz);

// Separate source: runs (entry of src[0, nsrc), destination entry, length) whose destinations tile [0, nnz) exactly.
CopyPlan build_copy_plan_from(std::vector<CopyRun> runs, int64_t nnz, int64_t nsrc);

// The kernel's lane logic on the host, work item by work item (every load of an item before its first store).
// stores: optional counters [nnz rounded up to whole spans], incremented for every entry a lane stores.
// src: the source buffer of a separate-source plan (every load is checked against [0, nsrc)); nullptr for a plan that
// copies inside vals.
void copy_plan_host_apply(const CopyPlan &plan, double *vals, int32_t *stores, const double *src = nullptr);

}  // namespace mha
