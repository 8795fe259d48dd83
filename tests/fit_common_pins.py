"""What csrc/fit_common.h holds for motion_fit.hip, epipolar.hip, superpixels.hip and two_view.hip, as source text: every shared
piece is defined there and nowhere else under csrc/, the telling line of each body occurs nowhere else (a copy under another name
would carry it), the names of the copies that were folded into it are gone, and the count of a wave's flagged lanes is
wave_ops.h's.  The ABI tests of the four stages call this."""
import os
import re

HEADER = "fit_common.h"
# the first words of each definition
DEFINITIONS = ("struct MfArgs {", "MfArgs fit_frame(", "int fit_clear(", "bool mf_part(", "void mf_load_model(", "uint32_t mf_grid_pixel(",
               "bool fit_draw(", "int fit_stage_chunk(", "void fit_block_add(", "unsigned long long fit_key(",
               "int fit_key_round(", "int fit_key_index(", "uint32_t fit_key_count(", "bool fit_offer(", "bool fit_adopt(",
               "void fit_counts(", "uint8_t fit_class(", "bool fit_scored(", "bool fit_affine_from_sums(",
               "#define FIT_THREADS 256\n", "#define FIT_CHUNK ", "#define FIT_ATTEMPTS 16\n", "#define FIT_PIVOT_MIN 9.094947017729282e-13 ",
               "#define FIT_DEGENERATE INT32_MIN\n", "#define FIT_NSUMS 12\n", "#define FIT_RANGE 32768.0f ")
# a line of each body: the Philox draw, the index from it, the compaction, the NaN pad, the key, its decode, the class byte, the
# cofactors and the back-conversion of step E, the power-of-two loop, the memset of d_state
BODIES = ("philox4x32_10(", "* (uint64_t)a.n) >> 32", "(slot >> 1) * 8 + (slot & 1)", '__builtin_nanf("")', "round * 65536 + j",
          "0xFFFFFFFFu - (uint32_t)key", "excluded ? 3 : in ? 1 : 2", "c00 = sbb * n - sb * sb", "(double)(h - 1)) * 0.015625", "P *= 2.0",
          "hipMemsetAsync(state, 0, 32 * sizeof(int64_t)")
# where a body line may also stand: the generator's own definition and the proposals that draw from it
ELSEWHERE = {"philox4x32_10(": {"philox.h", "neighbour.hip"}}
# the count of a wave's flagged lanes is wave_ops.h's: who calls it how often
WAVE_COUNTS = {"epipolar.hip": 4, "motion_fit.hip": 3}
GONE = ("fit_wave_count", "mf_block_add", "tv_block_add", "sf_affine", "MF_CHUNK", "EP_CHUNK", "MF_THREADS", "EP_THREADS", "MF_ATTEMPTS", "EP_ATTEMPTS",
        "MF_PIVOT_MIN", "EP_PIVOT_MIN", "MF_DEGENERATE", "EP_DEGENERATE", "MF_NSUMS", "SF_NSUMS", "MF_POLISH_RANGE", "SF_RANGE",
        "mf_f2", "ep_f2")
USERS = ("motion_fit.hip", "epipolar.hip", "superpixels.hip", "two_view.hip")


def check(csrc, *chunks):
    """Every pin above, and FIT_CHUNK equal to each of `chunks` (the CHUNK of the numpy restatements)."""
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h"))}
    for words in DEFINITIONS:
        assert [n for n, t in texts.items() if words in t] == [HEADER], words
        assert texts[HEADER].count(words) == 1, words
    for words in BODIES:
        assert {n for n, t in texts.items() if words in t} - ELSEWHERE.get(words, set()) == {HEADER}, words
    for name in GONE:
        assert not [n for n, t in texts.items() if re.search(r"\b%s\b" % name, t)], name
    for n in USERS:
        assert '#include "%s"' % HEADER in texts[n], n
    assert '#include "philox.h"' in texts[HEADER]
    # fit_common.h defines no wave count of its own: the seven flags of fit_block_add go through wave_ops.h's wave_count
    assert "__ballot(" not in texts[HEADER] and "__popcll(" not in texts[HEADER] and "int wave_count(" in texts["wave_ops.h"]
    for n, count in WAVE_COUNTS.items():
        assert texts[n].count("fit_block_add({wave_count(") == count and '#include "wave_ops.h"' in texts[n], n
    defines = [(n, m) for n, t in texts.items() for m in re.findall(r"#define FIT_CHUNK (\d+) ", t)]
    assert len(defines) == 1 and defines[0][0] == HEADER
    for chunk in chunks:
        assert int(defines[0][1]) == chunk
