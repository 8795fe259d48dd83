"""What cli.py and flowio.py hold for the eight argparse tools and run_batch.py, as source text: the parser construction, the
range, finiteness and extension checks, the refusal's print, the [U,V,valid] writer's channel swap and the class picture are written
nowhere in the tools any more; a tool fetches one sibling itself, cli; read_flow is defined once, in flowio.py; cli.py imports
the standard library only; and everything the tests call by name is still defined where they call it.  tests/test_cli.py calls this."""
import os
import re

TOOLS = ("flowfilter", "motionfit", "epipolar", "twoview", "superpixels", "tracks", "midframe", "flowpicture")
GONE = ("RawDescriptionHelpFormatter", "must lie in", "must be finite", "os.path.splitext", "[..., [1, 0]]", "* 85", "file=sys.stderr")
CLI_IMPORTS = {"argparse", "importlib", "json", "math", "os", "sys"}
# what the tests call by name, by file
DEFINED = dict({tool: ("parser()", "main(argv=None)") for tool in TOOLS},
               run_batch=("parser()", "main(argv=None)", "segments_arg(tokens)", "wmedian_arg(token)", "wmedian_reject_arg(tokens)",
                          "motion_args(a)", "epipolar_arg(a)", "pose_arg(a)", "midframe_args(a)"),
               spremiZaEpic=("take_segments(argv)",))
OWN = {"epipolar": ("def gated(flow, cls, np):", "MAX_HYP = "), "twoview": ("def camera(a):", "MAX_HYP = "),
       "superpixels": ("def label_picture(labels, np):", "def boundary_picture(img, labels, np):", "MAX_MIN_SIZE = "),
       "midframe": ("def count_line(t, counts):", "SOURCE_BGR = ")}


def check(package):
    texts = {n[:-3]: open(os.path.join(package, n)).read() for n in sorted(os.listdir(package)) if n.endswith(".py")}
    for name in TOOLS + ("run_batch",):
        for words in GONE:
            assert words not in texts[name], (name, words)
        assert texts[name].count("import_module(PKG") <= 1, name
    for name in TOOLS:
        assert texts[name].count('cli = importlib.import_module(PKG + ".cli")') == 1, name
        assert "sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))\nPKG = " in texts[name], name
    assert [n for n, t in texts.items() if "def read_flow" in t] == ["flowio"] and texts["flowio"].count("def read_flow(path):") == 1
    assert set(re.findall(r"^(?:import|from) (\w+)", texts["cli"], re.M)) <= CLI_IMPORTS
    assert not re.search(r"^\s+(?:import|from) ", texts["cli"], re.M), "no import inside a function either"
    for name, signatures in DEFINED.items():
        for sig in signatures:
            assert texts[name].count("\ndef %s:" % sig) == 1, (name, sig)
    for name, lines in OWN.items():
        for words in lines:
            assert texts[name].count("\n" + words) == 1, (name, words)
