// row_blocks_device.hpp -- the device copies of a RowBlocks partition (row_blocks.hpp) and the view the kernels take.
#pragma once
#include "common.hpp"
#include "kernels/device_types.hpp"
#include "row_blocks.hpp"

namespace mha {

struct RowBlocksOnDevice {
  DeviceBuffer<int32_t> row_ptr, rows, row_off, acc_size, elem_ptr, elems, pair_ptr, pair_off, row_base, row_len, emask, epbase;
  DeviceBuffer<int32_t> seg_ptr, seg_acc, seg_base, seg_len;
  DeviceBuffer<int64_t> slot_ptr;
  DeviceBuffer<uint32_t> pairs;

  // accumulator_tables = false leaves out what only the LDS-accumulator kernels read (row_off, acc_size, row_base, emask,
  // epbase): the view's pointers to them stay null
  void upload(const RowBlocks &rb, bool accumulator_tables = true) {
    RowBlocksDev &d = dev_;
    d = RowBlocksDev();
    d.num_blocks = rb.num_blocks;
    auto put = [](auto &buf, const auto &host, auto &ptr) { buf.upload(host); ptr = buf.data(); };
    put(row_ptr, rb.row_ptr, d.row_ptr);
    put(rows, rb.rows, d.rows);
    put(elem_ptr, rb.elem_ptr, d.elem_ptr);
    put(elems, rb.elems, d.elems);
    put(pair_ptr, rb.pair_ptr, d.pair_ptr);
    put(pairs, rb.pairs, d.pairs);
    put(pair_off, rb.pair_off, d.pair_off);
    put(row_len, rb.row_len, d.row_len);
    put(slot_ptr, rb.slot_ptr, d.slot_ptr);
    put(seg_ptr, rb.seg_ptr, d.seg_ptr);
    put(seg_acc, rb.seg_acc, d.seg_acc);
    put(seg_base, rb.seg_base, d.seg_base);
    put(seg_len, rb.seg_len, d.seg_len);
    if (accumulator_tables) {
      put(row_off, rb.row_off, d.row_off);
      put(acc_size, rb.acc_size, d.acc_size);
      put(row_base, rb.row_base, d.row_base);
      put(emask, rb.emask, d.emask);
      put(epbase, rb.epbase, d.epbase);
    }
    d.lds_rows = rb.max_rows;
    d.lds_elems = rb.max_elems;
    d.lds_acc = rb.max_acc;
    d.lds_pairs = rb.max_pairs;
    d.lds_segs = rb.max_segs;
  }
  RowBlocksDev dev() const { return dev_; }

 private:
  RowBlocksDev dev_;
};

}  // namespace mha
