"""What csrc/union_find.h and csrc/plane_ops.h hold for segments.hip, superpixels.hip and tracks.hip, as source text: the grid steps
of the component labelling, the leader loop, the in-block rank and the one-block scan are each defined once, in their header and
nowhere else under csrc/; the telling line of each body occurs nowhere else (a copy under another name would carry it; the scan
step and the rank below a lane are wave_ops.h's wave_scan_add and lane_rank); the copies that were folded into them are gone; every
kernel is still there under its own name.  The ABI tests of the three stages call this."""
import os
import re

# the first words of each definition, by header
DEFINITIONS = {"union_find.h": ("void uf_tile_step(", "int uf_border_joins(", "int uf_border_blocks(", "bool uf_border_pair(",
                                "void uf_root_step(", "int uf_find(", "void uf_union("),
               "plane_ops.h": ("void wave_each_key(", "void wave_add_by_key(", "int block_rank(", "int block_scan_sums(")}
# a line of each body: the leader pick, the scan's last step, the rank below a lane, the vertical- and horizontal-border index,
# the never-zero grid, the hang
BODIES = {"__ffsll((long long)todo) - 1": "plane_ops.h", "x += dpp_or0<DPP_ROW_BCAST31, 0xC>(x)": "wave_ops.h",
          "__builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)": "wave_ops.h", "(k % h) * w + (k / h + 1) *": "union_find.h",
          "- 1) * w + k % w": "union_find.h", "b > 0 ? b : 1": "union_find.h",
          "__hip_atomic_fetch_min(&L[start], x,": "union_find.h"}
# the tile-local root as a raster index, whatever the tile's constants are called
TILE_ROOT = re.compile(r"r / \w+\) \* w \+ .*r % \w+")
GONE = ("sp_wave_add",)
USERS = {"union_find.h": ("segments.hip", "superpixels.hip", "edges.hip"), "plane_ops.h": ("segments.hip", "tracks.hip", "union_find.h"),
         "wave_ops.h": ("plane_ops.h",)}
# every kernel keeps its file and its name, and is launched once in its launch function
KERNELS = {"segments.hip": ("seg_tile_kernel", "seg_border_kernel", "seg_root_kernel", "seg_write_kernel"),
           "superpixels.hip": ("sp_tile_kernel", "sp_border_kernel", "sp_root_kernel", "sp_merge_kernel", "sp_scan_kernel",
                               "sp_number_kernel", "sp_write_kernel", "sf_acc_kernel", "sf_solve_kernel", "sf_apply_kernel"),
           "tracks.hip": ("track_seed_count_kernel", "track_seed_scan_kernel", "track_seed_emit_kernel")}
# who calls what
CALLS = {"segments.hip": ("uf_tile_step<SEG_TW, SEG_TH>(", "uf_border_pair<SEG_TW, SEG_TH>(", "uf_border_blocks<SEG_TW, SEG_TH>(",
                          "uf_root_step<SEG_THREADS>("),
         "superpixels.hip": ("uf_tile_step<SP_TW, SP_TH>(", "uf_border_pair<SP_TW, SP_TH>(", "uf_border_blocks<SP_TW, SP_TH>(",
                             "uf_root_step<SP_THREADS>(", "wave_each_key(", "wave_add_by_key(agree,", "block_rank(final_root, s_fin)",
                             "block_scan_sums<SP_WAVES>("),
         "tracks.hip": ("block_rank(is[k], s_wave + k * TRK_WAVES)", "block_scan_sums<TRK_WAVES>("),
         "union_find.h": ("wave_add_by_key(root >= 0, root, size, 1)",)}


def check(csrc):
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h"))}
    body = lambda t, start: t[t.index(start):t.index("\n}\n", t.index(start))]                  # noqa: E731
    for header, names in DEFINITIONS.items():
        for words in names:
            assert [n for n, t in texts.items() if words in t] == [header], words
            assert texts[header].count(words) == 1, words
    for words, header in BODIES.items():
        assert [n for n, t in texts.items() if words in t] == [header] and texts[header].count(words) == 1, words
    assert [n for n, t in texts.items() if TILE_ROOT.search(t)] == ["union_find.h"] and len(TILE_ROOT.findall(texts["union_find.h"])) == 1
    for name in GONE:
        assert not [n for n, t in texts.items() if re.search(r"\b%s\b" % name, t)], name
    # the filler value of a pixel beyond the frame that nobody shares
    assert not [n for n, t in texts.items() if "-1 - t" in t]
    assert [n for n, t in texts.items() if "s_part[" in t] == ["plane_ops.h"]
    for header, users in USERS.items():
        for n in users:
            assert '#include "%s"' % header in texts[n], (header, n)
    for n, kernels in KERNELS.items():
        for k in kernels:
            assert len(re.findall(r"__global__ void __launch_bounds__\(\w+\) %s\(" % k, texts[n])) == 1, k
            assert texts[n].count("hipLaunchKernelGGL(%s," % k) == 1, k
    # the rank and the scan are built on the wave's
    assert "return (int)lane_rank(b);" in body(texts["plane_ops.h"], "int block_rank(")
    assert "(int)wave_scan_add((uint32_t)sum)" in body(texts["plane_ops.h"], "int block_scan_sums(")
    for n, calls in CALLS.items():
        for words in calls:
            assert words in texts[n], (n, words)
    # the helpers place no barrier but the tile step's pair and the scan's one: seed_block_flags keeps its single one for four rounds
    assert "__syncthreads" not in body(texts["plane_ops.h"], "int block_rank(")
    assert "__syncthreads" not in body(texts["plane_ops.h"], "void wave_each_key(")
    assert body(texts["tracks.hip"], "void seed_block_flags(").count("__syncthreads()") == 1
    assert body(texts["plane_ops.h"], "int block_scan_sums(").count("__syncthreads()") == 1
    assert body(texts["union_find.h"], "void uf_tile_step(").count("__syncthreads()") == 2
    # superpixels.hip takes the steps from the header and segments.hip knows nothing of its other user
    assert "superpixel" not in texts["segments.hip"] and "s_lab" not in texts["segments.hip"] + texts["superpixels.hip"]
