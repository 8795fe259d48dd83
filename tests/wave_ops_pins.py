"""What csrc/wave_ops.h holds for every file that works across the lanes of a wave, as source text: each primitive and each DPP
control word is defined once, there and nowhere else under csrc/; outside it nothing names the DPP builtin, a bare DPP control
number, an up shuffle, a butterfly loop or a counted ballot, except the sites listed below with their reasons; the names
that were folded into it are gone; every file that calls a primitive includes the header, which includes no project header; and
the kernels whose device code the move had to leave alone are still there under their names, launched where they were.  The ABI
tests of the library, the tracks, the superpixels and the motion fit call this."""
import os
import re

HEADER = "wave_ops.h"
# the first words of each definition
DEFINITIONS = ("#define DPP_QUAD_PERM(", "#define DPP_ROW_SHL(", "#define DPP_ROW_SHR(", "#define DPP_ROW_ROR(", "#define DPP_WAVE_SHR1 ",
               "#define DPP_ROW_HALF_MIRROR ", "#define DPP_ROW_BCAST15 ", "#define DPP_ROW_BCAST31 ", "int dpp_i(", "float dpp_f(",
               "uint32_t dpp_or0(", "int row_min16(", "int wave_min(", "uint32_t wave_scan_add(", "T wave_reduce_all(",
               "uint64_t wave_min_u64(", "uint64_t wave_max_u64(", "int wave_count(", "uint32_t lane_rank(",
               "void wave_lds_sync(")
# what only the header may say
HEADER_ONLY = ("__builtin_amdgcn_update_dpp", "__shfl_up(", "__popcll(__ballot(", "__builtin_amdgcn_wave_barrier(")
# the loop of a butterfly or a tree: it halves an offset from 32
BUTTERFLY = re.compile(r"for \(int \w+ = 32;[^)]*>>= 1\)")
# a DPP control word as a bare number in a template argument
BARE_CTRL = re.compile(r"<\s*0x1[0-4][0-9a-fA-F]\s*[,>]")
# the sites that stay as they were, by file: what stands there, how often, and why
EXCEPTIONS = {
    # one exchange between the two half-waves of the screen kernel, no reduction
    "knn_mfma.hip": {"__shfl_xor(": ("__shfl_xor(a5[gq][i], 32)", 1)},
    # bcd_lists_kernel's three ranks: lane_rank() there changes the kernel's instruction sequence (7881 -> 7868), and the kernel
    # is one of those that must keep theirs; the lines are lane_rank's body written out, with a comment that says so
    "bcd.hip": {"__builtin_amdgcn_mbcnt_hi(": ("__builtin_amdgcn_mbcnt_hi((uint32_t)(", 3)},
    # the lane-0 tree of block_reduce and of knn_jacobi_kernel: as a function of the header it gives mf_sums_kernel other device
    # code in every spelling tried, and the motion fit measured above the speed rule with it; both sites keep the parent's text
    "plane_ops.h": {"__shfl_down(": ("d[k] = __shfl_down(d[k], off, 64);", 1)},
    "knn_pca.hip": {"__shfl_down(": ("part += __shfl_down(part, off);", 1)},
}

GONE = ("fit_wave_count", "DPP_ROW_SHL1", "DPP_ROW_SHL2", "DPP_ROW_SHL4", "DPP_ROW_SHL8", "dpp_min")
# a call of a primitive, or a control word
PRIMITIVE = re.compile(r"\b(dpp_i|dpp_f|dpp_or0|row_min16|wave_min|wave_scan_add|wave_reduce_all|wave_min_u64|wave_max_u64|"
                       r"wave_count|lane_rank|wave_lds_sync)\s*[<(]|\bDPP_(QUAD_PERM|ROW_\w+|WAVE_SHR1)\b")
USERS = ("bcd.hip", "knn_mfma.hip", "epic.h", "plane_ops.h", "prior.hip", "label_conf.hip", "frame_interp.hip",
         "superpixels.hip", "two_view.hip", "epipolar.hip", "motion_fit.hip")
# who calls what: the sites that had a copy of their own
CALLS = {"plane_ops.h": ("wave_count(is[k])", "wave_count(mine)", "(int)lane_rank(b)",
                         "(int)wave_scan_add((uint32_t)sum)"),
         "knn_mfma.hip": ("m = wave_min_u64(m);", "(int)wave_scan_add((uint32_t)cntl)", "wave_min_u64(keys[0])", "wave_max_u64(entries)",
                          "dpp_f<CTRL>(mind)", "dpp_i<CTRL>(best)", "dpp_lexmin<DPP_ROW_SHL(8)>("),
         "epic.h": ("m = wave_min_u64(m);", "mx = wave_max_u64(mx);"),
         "superpixels.hip": ("wave_reduce_all(mine && part ? v[k] : 0ll,", "wave_count(mine && part)"),
         "bcd.hip": ("x[w] |= dpp_or0<CTRL, ROWS>(x[w]);", "sets_or_step<DPP_ROW_BCAST31, 0xC>(x)", "dpp_i<CTRL>(a.k)",
                     "cand_dpp<DPP_ROW_SHL(8)>(", "dpp_or0<DPP_WAVE_SHR1>(", "org[ax] = wave_min(mn);", "wave_scan_add(tot) - tot",
                     "lane_rank(moremask)", "wave_lds_sync();"),
         "prior.hip": ("wave_count(claimed)", "row_min16(m[k])", "dpp_f<DPP_ROW_HALF_MIRROR>(r)"),
         "label_conf.hip": ("row_min16(hi)",), "frame_interp.hip": ("wave_count(won)",),
         "two_view.hip": ("wave_count(cover[it])", "wave_count(vote[k])", "wave_count(k == q)")}
# what stays in its stage file: the kernels' own merges and the chain and lists kernels' own wave code
STAY = {"bcd.hip": ("void sets_or_step(", "void wave_scan_or(", "void cand_dpp(", "void wave_min_lane0(", "uint32_t wave_u32_min_asm(",
                    "unsigned long long wave_key_min_asm(", "struct Cand {"),
        "knn_mfma.hip": ("void dpp_lexmin(",)}
# the wait statements, by file
WAITS = {"bcd.hip": 1, "knn_mfma.hip": 8, "row_stage.h": 2}
# the kernels that keep their instruction sequence: file -> (kernel, launches); a launch is either spelling
KERNELS = {"bcd.hip": (("bcd_chain_kernel", 1), ("bcd_lists_kernel", 1)),
           "knn_mfma.hip": (("knn_screen_kernel", 1), ("knn_prep_kernel", 1), ("knn_resolve_kernel", 1), ("knn_finalize_kernel", 1)),
           "prior.hip": (("prior_kernel", 1),), "label_conf.hip": (("label_conf_kernel", 2),),
           "epic.hip": (("epic_init_kernel", 1), ("epic_voronoi_kernel", 1), ("epic_graph_count_kernel", 1), ("epic_graph_alloc_kernel", 1),
                        ("epic_graph_fill_kernel", 1), ("epic_lists_kernel", 1), ("epic_fill_kernel", 1)),
           "epic_prefilter.hip": (("pf_tensor_kernel", 1), ("pf_saliency_kernel", 1), ("pf_copy_kernel", 1), ("pf_consistency_kernel", 2),
                                  ("pf_compact_kernel", 1))}


def check(csrc):
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h"))}
    others = {n: t for n, t in texts.items() if n != HEADER}
    for words in DEFINITIONS:
        assert [n for n, t in texts.items() if words in t] == [HEADER], words
        assert texts[HEADER].count(words) == 1, words
    for words in HEADER_ONLY:
        assert not [n for n, t in others.items() if words in t], words
    # a loop that halves an offset from 32 is left only around the two trees listed below, so none is a butterfly
    assert {n: len(BUTTERFLY.findall(t)) for n, t in others.items() if BUTTERFLY.search(t)} == {"plane_ops.h": 1, "knn_pca.hip": 1}
    assert not [n for n, t in others.items() if BARE_CTRL.search(t)]
    # the listed sites, and no other, keep the words of a primitive's body
    for words in sorted({w for sites in EXCEPTIONS.values() for w in sites}):
        found = {n: t.count(words) for n, t in others.items() if words in t}
        assert found == {n: sites[words][1] for n, sites in EXCEPTIONS.items() if words in sites}, (words, found)
    for n, sites in EXCEPTIONS.items():
        for words, (site, count) in sites.items():
            assert texts[n].count(site) == count, (n, site)
    assert "wave_ops.h's lane_rank(mask) written out" in texts["bcd.hip"]
    # and the header holds no third copy of the tree
    assert "__shfl_down(" not in texts[HEADER] and not [n for n, t in texts.items() if "wave_reduce_down" in t]
    for name in GONE:
        assert not [n for n, t in texts.items() if re.search(r"\b%s\b" % name, t)], name
    # a file names a primitive exactly when it includes the header; the header itself includes the runtime and stdint alone
    strip = lambda t: re.sub(r"//[^\n]*", "", t)                                                   # noqa: E731
    assert sorted(n for n, t in others.items() if PRIMITIVE.search(strip(t))) == sorted(USERS)
    for n, t in others.items():
        assert ('#include "%s"' % HEADER in t) == (n in USERS), n
    assert re.findall(r"#include (\S+)", texts[HEADER]) == ["<hip/hip_runtime.h>", "<stdint.h>"]
    assert HEADER not in texts["dflow_common.h"]
    assert " wave_ops.h " in open(os.path.join(csrc, "Makefile")).read()
    for n, calls in CALLS.items():
        for words in calls:
            assert words in texts[n], (n, words)
    for n, names in STAY.items():
        for words in names:
            assert [m for m, t in texts.items() if words in t] == [n] and texts[n].count(words) == 1, words
    # every s_waitcnt statement of the kernels stays
    assert {n: t.count('asm volatile("s_waitcnt') for n, t in texts.items() if "s_waitcnt" in t} == WAITS
    for n, kernels in KERNELS.items():
        for k, launches in kernels:
            assert len(re.findall(r"__global__ void __launch_bounds__\([^)]*\) %s\(" % k, texts[n])) == 1, k
            assert len(re.findall(r"hipLaunchKernelGGL\(%s[,<]|\b%s(<\w+>)?<<<" % (k, k), texts[n])) == launches, k
            assert not [m for m, t in texts.items() if m != n and re.search(r"\b%s\b\s*[<(]" % k, strip(t))], k
