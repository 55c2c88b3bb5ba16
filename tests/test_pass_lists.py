"""A pass's pixel-list buffers (lists, row_counts, list_totals, part_cnt) have one compile-time layout
(dpe-mvs_amd/csrc/pass_lists.h): ensure_working_set allocates its totals and dpe_pm_execute takes every
pointer from it.  pass_lists_ok() checks bounds, pairwise overlap and the capacities the kernels need.
Here: the header compiles (its asserts hold), a layout whose failed list starts inside the all-WEAK
list does not, and the check holds at every shape up to 96 x 96."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "dpe-mvs_amd", "csrc", "pass_lists.h")


def _compile(tmp_path, body, *flags):
    src = tmp_path / "t.cpp"
    src.write_text(f'#include "{HDR}"\n{body}\n')
    return subprocess.run(["g++", "-std=c++17", *flags, str(src)], capture_output=True, text=True)


def test_layout_holds(tmp_path):
    # today's capacities: half-image lists px/2 + 64, the all-WEAK list px + 64; 7 half-image lists and
    # the all-WEAK one, nothing else, in `lists`
    r = _compile(tmp_path, "constexpr dpe::PassLists l(1600, 1200, 1200);\n"
                           "static_assert(l.sweep(1, 1).len == 960064 && l.sweep(1, 1).off == 3 * 960064, \"\");\n"
                           "static_assert(l.all_weak().len == 1920064 && l.side(1).len == 960064, \"\");\n"
                           "static_assert(l.lists_len() == 7 * 960064 + 1920064, \"\");\n"
                           "static_assert(l.failed_rows().off >= l.sweep_rows().off + l.sweep_rows().len, \"\");\n"
                           "static_assert(l.chunks() == 938 && l.part_cnt_len() == 2 * 938, \"\");\n"
                           "int main() { return 0; }", "-fsyntax-only")
    assert r.returncode == 0, r.stderr


def test_overlapping_layout_does_not_compile(tmp_path):
    # the failed-GenNeighbours list one entry inside the all-WEAK list: the aux stream would fill it
    # over the last WEAK pixel while GenNeighbours' successors still read that list
    layout = ("struct Shifted : dpe::PassLists {\n"
              "  using PassLists::PassLists;\n"
              "  constexpr Region failed() const { return {all_weak().off + all_weak().len - %d, half_cap(), 1}; }\n"
              "};\n"
              "DPE_PASS_LISTS_ASSERT(Shifted, 12, 40, 40);\n"
              "int main() { return 0; }")
    r = _compile(tmp_path, layout % 1, "-fsyntax-only")
    assert r.returncode != 0 and "pass-list layout at 12x40" in r.stderr, r.stderr
    assert _compile(tmp_path, layout % 0, "-fsyntax-only").returncode == 0   # the same type, not shifted


def test_layout_holds_at_every_small_shape(tmp_path):
    # half_rows as in compute_pass_constants (dpe_mvs.hip)
    prog = ("#include <algorithm>\n"
            "int main() {\n"
            "  for (int W = 1; W <= 96; ++W)\n"
            "    for (int H = 1; H <= 96; ++H) {\n"
            "      const int half_rows = std::min(H, 2 * 16 * (((H / 2) + 15) / 16));\n"
            "      if (!dpe::pass_lists_ok(dpe::PassLists(W, H, half_rows))) return 1;\n"
            "    }\n"
            "  return dpe::pass_lists_ok(dpe::PassLists(12, 40, 41)) ? 2 : 0;   // rows outside the image: refused\n"
            "}")
    exe = tmp_path / "t"
    r = _compile(tmp_path, prog, "-O1", "-o", str(exe))
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
