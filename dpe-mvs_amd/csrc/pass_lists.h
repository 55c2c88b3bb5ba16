// pass_lists.h — the one layout of a pass's pixel-list buffers (DpeContext::lists, row_counts,
// list_totals, part_cnt): ensure_working_set allocates its totals, dpe_pm_execute takes every
// pointer from it, dpe_pm_last_stat reads its named slot.
//
// Every region is (offset, capacity) in ints, an lds::Region with alignment 1.  pass_lists_ok()
// checks at compile time, with lds::regions_ok, that each region lies inside its buffer and overlaps
// no other, and that the capacities cover what the kernels touch; the header asserts it at the shapes
// below.  Pure C++ (no HIP types): tests/test_pass_lists.py compiles it with g++, shows that an
// overlapping layout does not compile, and runs the check over every small shape.
#pragma once
#include <climits>

#include "lds_layout.h"

namespace dpe {

constexpr int kPartChunk = 1024;   // entries per chunk of the weak-list partition (pass_sweep.h, k_part_*)

struct PassLists {
  using Region = lds::Region;
  int W, H, half_rows;   // half_rows: rows of the red/black grid (compute_pass_constants)
  constexpr PassLists(int W_, int H_, int half_rows_) : W(W_), H(H_), half_rows(half_rows_) {}
  constexpr long px() const { return (long)W * H; }

  // ---- lists: pixel indices.  A half-image list holds at most px/2 + 1 pixels; the sweeps read up
  // to one wave's pixels past the count, inside the 64-entry slack.  The four sweep lists are
  // consecutive at stride half_cap(): k_list_fill<0> writes list k = colour*2 + cls at k * stride.
  constexpr int half_cap() const { return (int)(px() / 2 + 64); }
  constexpr Region sweep(int colour, int cls) const { return {(colour * 2 + cls) * half_cap(), half_cap(), 1}; }   // cls 0 strong, 1 weak
  constexpr Region all_weak() const { return {4 * half_cap(), (int)(px() + 64), 1}; }   // every WEAK pixel, for GenNeighbours
  constexpr Region failed() const { return {all_weak().off + all_weak().len, half_cap(), 1}; }   // colour-0 pixels whose GenNeighbours failed
  constexpr Region side(int colour) const { return {failed().off + (1 + colour) * half_cap(), half_cap(), 1}; }   // a colour's weak list by patch side
  constexpr long lists_len() const { return 7L * half_cap() + px() + 64; }

  // ---- row_counts: per-row counts, then offsets, of each list build (k_list_count/scan/fill<MODE>);
  // k_list_*<0> index the four sweep lists' rows as [k * half_rows + y]
  constexpr Region sweep_rows() const { return {0, 4 * half_rows, 1}; }
  constexpr Region all_weak_rows() const { return {4 * half_rows, H, 1}; }
  constexpr Region failed_rows() const { return {4 * half_rows + H, half_rows, 1}; }
  constexpr int row_counts_len() const { return 5 * half_rows + H; }

  // ---- list_totals: one int per list; k_list_scan<0> writes the sweep lists' four as [k]
  static constexpr int kTotSweep = 0, kTotAllWeak = 4, kTotFailed = 5, kTotGnOverflow = 6, kTotSide = 7, kTotals = 9;
  static constexpr int total_sweep(int colour, int cls) { return kTotSweep + colour * 2 + cls; }
  static constexpr int total_side(int colour) { return kTotSide + colour; }   // side >= 4 entries of side(colour)

  // ---- part_cnt: per colour, the chunk counts / offsets of the weak-list partition (k_part_*)
  constexpr int chunks() const { return (int)((px() / 2 + 1 + kPartChunk - 1) / kPartChunk); }
  constexpr Region chunk_counts(int colour) const { return {colour * chunks(), chunks(), 1}; }
  constexpr int part_cnt_len() const { return 2 * chunks(); }
};

// Layout: PassLists, or a type with its interface (the test's deliberately broken one).
template <class Layout>
constexpr bool pass_lists_ok(const Layout& l) {
  // (half_rows == 0: an image of one row has no red/black row)
  if (l.W < 1 || l.H < 1 || l.half_rows < 0 || l.half_rows > l.H || l.lists_len() > INT_MAX) return false;
  const long half = l.px() / 2 + 1;   // most pixels of one colour
  const lds::Region lists[] = {l.sweep(0, 0), l.sweep(0, 1), l.sweep(1, 0), l.sweep(1, 1),
                               l.all_weak(),  l.failed(),    l.side(0),     l.side(1)};
  const lds::Region rows[] = {l.sweep_rows(), l.all_weak_rows(), l.failed_rows()};
  const lds::Region totals[] = {{l.total_sweep(0, 0), 1, 1}, {l.total_sweep(0, 1), 1, 1}, {l.total_sweep(1, 0), 1, 1},
                                {l.total_sweep(1, 1), 1, 1}, {Layout::kTotAllWeak, 1, 1},       {Layout::kTotFailed, 1, 1},
                                {Layout::kTotGnOverflow, 1, 1},    {l.total_side(0), 1, 1},     {l.total_side(1), 1, 1}};
  const lds::Region chunks[] = {l.chunk_counts(0), l.chunk_counts(1)};
  if (!lds::regions_ok(lists, (int)l.lists_len()) || !lds::regions_ok(rows, l.row_counts_len()) ||
      !lds::regions_ok(totals, Layout::kTotals) || !lds::regions_ok(chunks, l.part_cnt_len()))
    return false;
  for (int k = 0; k < 4; ++k) {   // k_list_*<0>: consecutive lists, rows and totals; a wave of slack
    if (lists[k].len < half + 63 || lists[k].off != lists[0].off + k * lists[0].len) return false;
    if (l.total_sweep(k >> 1, k & 1) != l.total_sweep(0, 0) + k) return false;
  }
  for (int k = 5; k < 8; ++k) if (lists[k].len < half + 63) return false;
  if (lists[4].len < l.px() + 63 || rows[0].len < 4 * l.half_rows || rows[1].len < l.H || rows[2].len < l.half_rows) return false;
  for (int k = 0; k < 2; ++k) if (chunks[k].len < (half + kPartChunk - 1) / kPartChunk) return false;
  return true;
}

// the message the failing layout of tests/test_pass_lists.py is recognised by
#define DPE_PASS_LISTS_ASSERT(Layout, W, H, HALF_ROWS)                 \
  static_assert(dpe::pass_lists_ok(Layout(W, H, HALF_ROWS)),           \
                "pass-list layout at " #W "x" #H ": a region overlaps another, leaves its buffer or is too small")
DPE_PASS_LISTS_ASSERT(PassLists, 1, 1, 1);
DPE_PASS_LISTS_ASSERT(PassLists, 12, 40, 40);
DPE_PASS_LISTS_ASSERT(PassLists, 77, 33, 32);
DPE_PASS_LISTS_ASSERT(PassLists, 193, 29, 29);
DPE_PASS_LISTS_ASSERT(PassLists, 1600, 1200, 1200);
DPE_PASS_LISTS_ASSERT(PassLists, 1920, 1080, 1080);
DPE_PASS_LISTS_ASSERT(PassLists, 16000, 16000, 16000);   // the largest image dpe_pm_stage accepts: offsets fit an int

}  // namespace dpe
