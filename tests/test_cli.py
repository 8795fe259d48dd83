"""The command-line layer (CPU only): cli.py's checks at their edges, flowio's flow reader and its field and grey writers, the
transcript of every refusal the tools and run_batch.py make, no torch on the way to a refusal, and the source pins."""
import contextlib
import io
import os
import re
import runpy
import subprocess
import sys

import numpy as np
import pytest

import cli_pins
from conftest import PKG, ROOT, pkg

NAN, INF = float("nan"), float("inf")


def refused(capsys, check, name, *args):
    """check(ap, name, *args) exits through ap.error: status 2, "error:" and the option's name on stderr."""
    with pytest.raises(SystemExit) as e:
        check(pkg("cli").parser("a tool"), name, *args)
    err = capsys.readouterr().err
    return e.value.code == 2 and "error:" in err and name in err


def test_the_checks_at_their_edges(capsys):
    cli = pkg("cli")
    ap = cli.parser("a tool")
    for v in (3, 9, None):
        cli.in_range(ap, "--n", v, 3, 9)
    for v in (2, 10):
        assert refused(capsys, cli.in_range, "--n", v, 3, 9), v
    assert refused(capsys, cli.in_range, "--seed", -1, 0, 2 ** 64 - 1) and refused(capsys, cli.in_range, "--seed", 2 ** 64, 0, 2 ** 64 - 1)
    cli.in_range(ap, "--seed", 2 ** 64 - 1, 0, 2 ** 64 - 1)
    for v in (5e-324, 1e308, None):
        cli.positive(ap, "--x", v)
    for v in (0.0, -0.0, -1, NAN, INF, -INF):
        assert refused(capsys, cli.positive, "--x", v), v
    for v in (0.0, -0.0, 5e-324, None):
        cli.non_negative(ap, "--x", v)
    for v in (-5e-324, NAN, INF, -INF):
        assert refused(capsys, cli.non_negative, "--x", v), v
    for v in (5e-324, 0.5, 1 - 2.0 ** -53, None):
        cli.between(ap, "--t", v, 0.0, 1.0)
    for v in (0.0, 1.0, NAN, INF):
        assert refused(capsys, cli.between, "--t", v, 0.0, 1.0), v
    for path in ("X.FLO", "x.flo", "dir.npy/x.Flo", None):
        cli.extension(ap, "--out", path, ".flo")
    cli.extension(ap, "--out", "x.NPY", ".flo", ".npy")
    for path in ("x", "x.flo.txt", "x.png", ".flo", "x.flo/y"):
        assert refused(capsys, cli.extension, "--out", path, ".flo", ".npy"), path


def test_the_token_form_raises_and_never_exits():
    cli = pkg("cli")
    assert cli.integer("8", 1, 8) == 8 and cli.integer(" 1 ", 1, 8) == 1 and cli.integer(5, 1, 8) == 5
    for token in ("x", "", "nan", "1.5", "0", "9", "-1"):
        with pytest.raises(ValueError):
            cli.integer(token, 1, 8)
    with pytest.raises(ValueError, match=r"^must lie in \[1, 8\]$"):
        cli.integer("9", 1, 8)
    assert cli.real("5e-324", True) == 5e-324 and cli.real("0", False) == 0.0 and cli.real("-0.0", False) == 0.0
    assert cli.real("-3", None) == -3.0 and cli.real(2.5, True) == 2.5
    for token, positive in (("x", True), ("", True), ("nan", True), ("0", True), ("-0.0", True), ("inf", True), ("-1", True),
                            ("x", False), ("", False), ("nan", False), ("-5e-324", False), ("inf", False),
                            ("x", None), ("nan", None), ("inf", None), ("-inf", None)):
        with pytest.raises(ValueError):
            cli.real(token, positive)
    with pytest.raises(ValueError, match="^must be finite and > 0$"):
        cli.real("0", True)
    with pytest.raises(ValueError, match="^must be finite and >= 0$"):
        cli.real("-1", False)
    assert cli.segments(["20", "1"]) == (20, 1.0) and cli.segments(["0", "0", "more"]) == (0, 0.0)
    assert cli.segments([str(2 ** 31 - 1), "0.5"]) == (2 ** 31 - 1, 0.5)
    for tokens in ([], ["20"], ["20", "x"], ["2.5", "1"], ["-1", "1"], ["20", "-1"], ["20", "nan"], ["20", "inf"], [str(2 ** 31), "1"]):
        with pytest.raises(ValueError, match=r"^--segments needs MIN \(an integer >= 0\) and T \(finite, >= 0\), got \["):
            cli.segments(tokens)


def test_the_refusal_and_the_report(capsys):
    cli = pkg("cli")
    assert cli.refuse("tool", OSError(2, "No such file or directory", "f.flo")) == 2
    assert capsys.readouterr() == ("", "tool: [Errno 2] No such file or directory: 'f.flo'\n")
    assert cli.REFUSED == (ValueError, OSError)
    cli.report(True, {"a": 1, "b": [0.5, None]}, ["never"])
    cli.report(False, {"a": 1}, ["one", "two"])
    assert capsys.readouterr() == ('{"a": 1, "b": [0.5, null]}\none\ntwo\n', "")
    assert cli.inliers(1, 3, True) == (1 / 3, "inliers: 1 of 3 scored vectors (33.33%)")
    assert cli.inliers(0, 0, False) == (0.0, "inliers: 0 of 0 scored vectors (0.00%); no model was found")


def test_read_flow(tmp_path):
    flowio = pkg("flowio")
    uv = np.arange(24, dtype=np.float32).reshape(3, 4, 2)
    uv[0, 0] = (-0.0, np.float32(0.1))
    flowio.write_flo(str(tmp_path / "f.flo"), uv)                           # takes [dy,dx]
    got = flowio.read_flow(str(tmp_path / "f.flo"))
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.tobytes() == uv.tobytes()
    assert flowio.read_flo(str(tmp_path / "f.flo")).tobytes() == np.ascontiguousarray(uv[..., ::-1]).tobytes()
    f64 = np.arange(24, dtype=np.float64).reshape(3, 4, 2) / 7
    np.save(tmp_path / "f2.npy", f64)
    got = flowio.read_flow(str(tmp_path / "f2.npy"))
    assert got.dtype == np.float32 and got.shape == (3, 4, 2) and got.tobytes() == f64.astype(np.float32).tobytes()
    f3 = np.arange(36, dtype=np.float32).reshape(3, 4, 3)
    with open(tmp_path / "F3.NPY", "wb") as f:                              # np.save would append '.npy' to this name
        np.save(f, f3)
    assert flowio.read_flow(str(tmp_path / "F3.NPY")).tobytes() == f3.tobytes()
    for shape in ((3, 4), (3, 4, 4)):
        np.save(tmp_path / "bad.npy", np.zeros(shape))
        with pytest.raises(ValueError, match=re.escape("bad.npy: expected an (H,W,2) or (H,W,3) array, got %s" % (shape,))):
            flowio.read_flow(str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError, match="^unsupported flow file: .*f.txt$"):
        flowio.read_flow(str(tmp_path / "f.txt"))
    with pytest.raises(OSError, match="No such file or directory"):
        flowio.read_flow(str(tmp_path / "missing.flo"))
    with pytest.raises(OSError, match="No such file or directory"):
        flowio.read_flow(str(tmp_path / "missing.npy"))


def test_the_field_writer_and_the_grey_writer(tmp_path):
    flowio = pkg("flowio")
    base = np.zeros((3, 5, 6), np.float32)
    field = base[..., ::2]                                                  # a view, not contiguous
    field[...] = np.arange(45, dtype=np.float32).reshape(3, 5, 3) - 7
    field[..., 2] = 1.0
    field[0, 0] = (-0.0, 0.0, 1.0)
    field[1, 2, :2].view(np.uint32)[:] = (0x7FC01234, 0xFFC00001)           # NaNs with payloads
    field[2, 4] = (3.5, -4.5, 0.0)                                          # invalid pixels that still hold numbers
    field[0, 3] = 0.0
    assert not field.flags.c_contiguous
    want = np.ascontiguousarray(field)
    flowio.write_field(str(tmp_path / "f.npy"), field)
    got = np.load(tmp_path / "f.npy")
    assert got.dtype == np.float32 and got.shape == (3, 5, 3) and got.tobytes() == want.tobytes()
    flowio.write_field(str(tmp_path / "F.FLO"), field)
    assert flowio.read_flo(str(tmp_path / "F.FLO")).tobytes() == np.ascontiguousarray(want[..., :2]).tobytes()
    # the bytes of the call it replaces
    flowio.write_flo(str(tmp_path / "old.flo"), want[..., [1, 0]])
    assert open(tmp_path / "F.FLO", "rb").read() == open(tmp_path / "old.flo", "rb").read()
    # the grey pictures: four classes with step 85, K layers with 255 // K
    classes = np.array([[0, 1], [2, 3], [3, 0]], np.uint8)
    flowio.write_grey(str(tmp_path / "c.png"), classes, 85)
    pic = flowio.read_png8(str(tmp_path / "c.png"))
    assert pic.shape == (3, 2, 3) and pic.dtype == np.uint8
    for ch in range(3):
        assert pic[..., ch].tolist() == [[0, 85], [170, 255], [255, 0]]
    for k in (1, 3, 7, 255):
        layers = np.arange(k + 1, dtype=np.uint8).reshape(1, -1)
        flowio.write_grey(str(tmp_path / "l.png"), layers, 255 // k)
        pic = flowio.read_png8(str(tmp_path / "l.png"))
        for ch in range(3):
            assert pic[0, :, ch].tolist() == [i * (255 // k) for i in range(k + 1)], k
    assert flowio.numbered_name("dir.x/out.png", 7) == "dir.x/out_07.png" and flowio.numbered_name("out", 12) == "out_12"


def run_tool(tool, argv, monkeypatch):
    """(the exit status, the last line of stderr without argparse's program name) of one command line, run in this process."""
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        try:
            if tool == "daisy i flann":
                monkeypatch.setattr(sys, "argv", [tool + ".py"] + argv)
                runpy.run_path(os.path.join(ROOT, PKG, tool + ".py"), run_name="__main__")
                status = 0
            elif tool == "python bcd":
                status = runpy.run_path(os.path.join(ROOT, PKG, tool + ".py"), run_name="bcd_cli")["main"](argv)
            else:
                status = pkg(tool).main(argv)
        except SystemExit as e:
            status = e.code
    lines = err.getvalue().strip().splitlines()
    return status, re.sub(r"^.*?: error: ", "error: ", lines[-1]) if lines else ""


def test_the_transcript_of_every_refusal(tmp_path, monkeypatch):
    """Every command line the test_command_line_refusals tests try, with the unreadable and ill-fitting inputs they make: the
    status is 2 and the last line of stderr is the one recorded from the commit before cli.py, but for three lines that now
    carry the shared helper's wording (<out> of flowfilter.py, --cap of tracks.py twice)."""
    monkeypatch.chdir(tmp_path)
    flowio = pkg("flowio")
    for name in ("i.png", "a.png", "b.png"):
        flowio.write_png8(name, np.zeros((6, 8, 3), np.uint8))
    for name, array in (("f.npy", np.zeros((6, 9, 2))), ("g.npy", np.zeros((6, 9))), ("bad.npy", np.zeros((6, 9), np.float32)),
                        ("f0.npy", np.zeros((6, 9, 2), np.float32)), ("f1.npy", np.zeros((6, 8, 2), np.float32)),
                        ("i.npy", np.zeros((6, 9, 3), np.uint8)), ("m64.npy", np.zeros((6, 9))), ("m.npy", np.zeros((6, 8), np.float32))):
        np.save(name, array)
    before = sorted(os.listdir("."))
    n = 0
    for tool, prefix, cases in TRANSCRIPT:
        for tail, last in cases:
            assert run_tool(tool, prefix + tail, monkeypatch) == (2, last), (tool, prefix + tail)
            n += 1
    assert n == 264 and sorted(os.listdir(".")) == before, "a refusal writes nothing"


USAGE = {"flowfilter": ["f.npy", "o.flo", "--radius", "0"], "motionfit": ["f.npy", "--thresh", "nan"], "epipolar": ["f.npy", "--hyp", "0"],
         "twoview": ["f.npy", "--focal", "0"], "superpixels": ["i.png", "o.npy", "--step", "3"], "tracks": ["f0.flo", "--out", "t.npy"],
         "midframe": ["a.png", "b.png", "f.npy", "out.png", "--t", "0"], "flowpicture": ["f.flo"]}
MISSING = {"flowfilter": ["missing.flo", "o.flo"], "motionfit": ["missing.flo"], "epipolar": ["missing.npy"], "twoview": ["missing.flo"],
           "superpixels": ["missing.png", "o.npy"], "tracks": ["missing.flo", "--out", "t.npz"]}
CHILD = "import runpy, sys; sys.modules['torch'] = None; del sys.argv[0]; runpy.run_path(sys.argv[0], run_name='__main__')"


@pytest.mark.parametrize("start,tool,argv", [("%s.py: error: ", t, a) for t, a in USAGE.items()] + [("%s: [Errno 2]", t, a) for t, a in MISSING.items()])
def test_a_refusal_never_imports_torch(start, tool, argv, tmp_path):
    """The script itself in a child process in which `import torch` fails: a refusal still ends with status 2 and its line."""
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, PKG, tool + ".py")] + argv, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and r.stdout == "" and "Traceback" not in r.stderr, r.stderr
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith(start % tool), last
    assert os.listdir(tmp_path) == []


def test_cli_imports_the_standard_library_only():
    code = "import sys; sys.modules['numpy'] = sys.modules['torch'] = None; sys.path.insert(0, %r); import importlib; " \
           "importlib.import_module(%r + '.cli'); print(sorted(m for m in sys.modules if m.startswith(%r)))" % (ROOT, PKG, PKG)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == repr([PKG, PKG + ".cli"]), r.stderr


def test_the_source_pins():
    cli_pins.check(os.path.join(ROOT, PKG))


# Recorded from the commit before cli.py; status 2 throughout.  (tool, the leading tokens, ((the rest, the last line of stderr), ...))
TRANSCRIPT = (
    ("flowfilter", ["f.npy", "o.flo"], (
        (["--radius", "0"], "error: --radius must lie in [1, 8]"),
        (["--radius", "9"], "error: --radius must lie in [1, 8]"),
        (["--sigma-space", "0"], "error: --sigma-space must be finite and > 0"),
        (["--sigma-space", "nan"], "error: --sigma-space must be finite and > 0"),
        (["--sigma-color", "-1"], "error: --sigma-color must be finite and > 0"),
        (["--sigma-color", "inf"], "error: --sigma-color must be finite and > 0"),
        (["--iterations", "0"], "error: --iterations must lie in [1, 16]"),
        (["--iterations", "17"], "error: --iterations must lie in [1, 16]"),
        (["--reject", "-1"], "error: --reject must be finite and >= 0"),
        (["--reject", "nan"], "error: --reject must be finite and >= 0"),
        (["--reject", "inf"], "error: --reject must be finite and >= 0"),
        (["--reject", "1", "--iterations", "2"], "error: --reject goes with one pass, not with --iterations"),
        (["--radius", "x"], "error: argument --radius: invalid int value: 'x'"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
    )),
    ("flowfilter", [], (
        ([], "error: the following arguments are required: flow, out"),
        (["f.npy"], "error: the following arguments are required: out"),
        (["f.npy", "o.png"], "error: <out> must be a .flo or .npy file"),
    )),
    ("flowfilter", [], (
        (["f.npy", "o.flo", "--image", "i.png"], "flowfilter: the flow is 9x6 and the image 8x6"),
        (["g.npy", "o.flo"], "flowfilter: g.npy: expected an (H,W,2) or (H,W,3) array, got (6, 9)"),
        (["missing.flo", "o.flo"], "flowfilter: [Errno 2] No such file or directory: 'missing.flo'"),
        (["f.txt", "o.flo"], "flowfilter: unsupported flow file: f.txt"),
    )),
    ("run_batch", [], (
        (["--wmedian", "0"], "error: --wmedian needs R (an integer in 1..8), got '0'"),
        (["--wmedian", "9"], "error: --wmedian needs R (an integer in 1..8), got '9'"),
        (["--wmedian", "x"], "error: --wmedian needs R (an integer in 1..8), got 'x'"),
        (["--wmedian", "1.5"], "error: --wmedian needs R (an integer in 1..8), got '1.5'"),
        (["--wmedian-reject", "0", "1"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['0', '1']"),
        (["--wmedian-reject", "9", "1"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['9', '1']"),
        (["--wmedian-reject", "3", "-1"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['3', '-1']"),
        (["--wmedian-reject", "3", "nan"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['3', 'nan']"),
        (["--wmedian-reject", "3", "inf"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['3', 'inf']"),
        (["--wmedian-reject", "3"], "error: argument --wmedian-reject: expected 2 arguments"),
        (["--wmedian-reject", "a", "1"], "error: --wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0), got ['a', '1']"),
    )),
    ("motionfit", ["f.npy"], (
        (["--model", "rigid"], "error: argument --model: invalid choice: 'rigid' (choose from 'affine', 'homography')"),
        (["--thresh", "0"], "error: --thresh must be finite and > 0"),
        (["--thresh", "nan"], "error: --thresh must be finite and > 0"),
        (["--thresh", "inf"], "error: --thresh must be finite and > 0"),
        (["--thresh", "-1"], "error: --thresh must be finite and > 0"),
        (["--hyp", "0"], "error: --hyp must lie in [1, 65536]"),
        (["--hyp", "65537"], "error: --hyp must lie in [1, 65536]"),
        (["--lo-rounds", "5"], "error: --lo-rounds must lie in [0, 4]"),
        (["--lo-rounds", "-1"], "error: --lo-rounds must lie in [0, 4]"),
        (["--polish", "5"], "error: --polish must lie in [0, 4]"),
        (["--step", "0"], "error: --step must lie in [1, 64]"),
        (["--step", "65"], "error: --step must lie in [1, 64]"),
        (["--seed", "-1"], "error: --seed must lie in [0, 18446744073709551615]"),
        (["--layers", "0"], "error: --layers must lie in [1, 255]"),
        (["--layers", "256"], "error: --layers must lie in [1, 255]"),
        (["--layers", "2", "--model-flow", "m.flo"], "error: --model-flow and --residual describe one model: they do not go with --layers"),
        (["--layers", "2", "--residual", "r.flo"], "error: --model-flow and --residual describe one model: they do not go with --layers"),
        (["--model-flow", "m.npy"], "error: --model-flow must be a .flo file"),
        (["--residual", "r.png"], "error: --residual must be a .flo file"),
        (["--classes", "c.flo"], "error: --classes must be a .png file"),
        (["--hyp", "x"], "error: argument --hyp: invalid int value: 'x'"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
    )),
    ("motionfit", [], (
        ([], "error: the following arguments are required: flow"),
        (["g.npy"], "motionfit: g.npy: expected an (H,W,2) or (H,W,3) array, got (6, 9)"),
        (["missing.flo"], "motionfit: [Errno 2] No such file or directory: 'missing.flo'"),
        (["f.txt"], "motionfit: unsupported flow file: f.txt"),
    )),
    ("run_batch", [], (
        (["--motion", "rigid"], "error: --motion needs MODEL (affine or homography), got 'rigid'"),
        (["--motion", "0"], "error: --motion needs MODEL (affine or homography), got '0'"),
        (["--motion", "affine", "--motion-thresh", "0"], "error: --motion-thresh needs T (finite, > 0), got '0'"),
        (["--motion", "affine", "--motion-thresh", "nan"], "error: --motion-thresh needs T (finite, > 0), got 'nan'"),
        (["--motion", "affine", "--motion-thresh", "inf"], "error: --motion-thresh needs T (finite, > 0), got 'inf'"),
        (["--motion", "affine", "--motion-thresh", "x"], "error: --motion-thresh needs T (finite, > 0), got 'x'"),
        (["--motion-thresh", "1"], "error: --motion-thresh needs --motion"),
        (["--motion"], "error: argument --motion: expected one argument"),
    )),
    ("epipolar", ["f.npy"], (
        (["--thresh", "0"], "error: --thresh must be finite and > 0"),
        (["--thresh", "nan"], "error: --thresh must be finite and > 0"),
        (["--thresh", "inf"], "error: --thresh must be finite and > 0"),
        (["--thresh", "-1"], "error: --thresh must be finite and > 0"),
        (["--hyp", "0"], "error: --hyp must lie in [1, 21845]"),
        (["--hyp", "21846"], "error: --hyp must lie in [1, 21845]"),
        (["--lo-rounds", "5"], "error: --lo-rounds must lie in [0, 4]"),
        (["--lo-rounds", "-1"], "error: --lo-rounds must lie in [0, 4]"),
        (["--step", "0"], "error: --step must lie in [1, 64]"),
        (["--step", "65"], "error: --step must lie in [1, 64]"),
        (["--seed", "-1"], "error: --seed must lie in [0, 18446744073709551615]"),
        (["--classes", "c.flo"], "error: --classes must be a .png file"),
        (["--residual", "r.flo"], "error: --residual must be a .npy file"),
        (["--gate", "g.png"], "error: --gate must be a .flo or .npy file"),
        (["--hyp", "x"], "error: argument --hyp: invalid int value: 'x'"),
        (["--polish", "1"], "error: unrecognized arguments: --polish 1"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
    )),
    ("epipolar", [], (
        ([], "error: the following arguments are required: flow"),
        (["g.npy"], "epipolar: g.npy: expected an (H,W,2) or (H,W,3) array, got (6, 9)"),
        (["missing.flo"], "epipolar: [Errno 2] No such file or directory: 'missing.flo'"),
        (["f.txt"], "epipolar: unsupported flow file: f.txt"),
    )),
    ("run_batch", [], (
        (["--epipolar", "0"], "error: --epipolar needs T (finite, > 0), got '0'"),
        (["--epipolar", "nan"], "error: --epipolar needs T (finite, > 0), got 'nan'"),
        (["--epipolar", "inf"], "error: --epipolar needs T (finite, > 0), got 'inf'"),
        (["--epipolar", "x"], "error: --epipolar needs T (finite, > 0), got 'x'"),
        (["--epipolar-gate"], "error: --epipolar-gate needs --epipolar"),
        (["--epipolar"], "error: argument --epipolar: expected one argument"),
    )),
    ("twoview", ["f.npy"], (
        (["--thresh", "0"], "error: --thresh must be finite and > 0"),
        (["--thresh", "nan"], "error: --thresh must be finite and > 0"),
        (["--hyp", "0"], "error: --hyp must lie in [1, 21845]"),
        (["--hyp", "21846"], "error: --hyp must lie in [1, 21845]"),
        (["--lo-rounds", "5"], "error: --lo-rounds must lie in [0, 4]"),
        (["--step", "0"], "error: --step must lie in [1, 64]"),
        (["--step", "65"], "error: --step must lie in [1, 64]"),
        (["--seed", "-1"], "error: --seed must lie in [0, 18446744073709551615]"),
        (["--focal", "0"], "error: --focal must be finite and > 0"),
        (["--focal", "nan"], "error: --focal must be finite and > 0"),
        (["--focal", "inf"], "error: --focal must be finite and > 0"),
        (["--focal", "-2"], "error: --focal must be finite and > 0"),
        (["--focal", "x"], "error: argument --focal: invalid float value: 'x'"),
        (["--intrinsics", "1", "2", "3"], "error: argument --intrinsics: expected 4 arguments"),
        (["--intrinsics", "0", "1", "2", "3"], "error: --intrinsics: FX and FY must be finite and > 0, CX and CY finite"),
        (["--intrinsics", "1", "1", "nan", "3"], "error: --intrinsics: FX and FY must be finite and > 0, CX and CY finite"),
        (["--intrinsics", "1", "inf", "2", "3"], "error: --intrinsics: FX and FY must be finite and > 0, CX and CY finite"),
        (["--focal", "5", "--intrinsics", "1", "1", "2", "3"], "error: argument --intrinsics: not allowed with argument --focal"),
        (["--depth", "d.png"], "error: --depth must be a .npy file"),
        (["--classes", "c.npy"], "error: --classes must be a .png file"),
        (["--err", "e.flo"], "error: --err must be a .npy file"),
        (["--gate", "g.npy"], "error: unrecognized arguments: --gate g.npy"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
    )),
    ("twoview", [], (
        ([], "error: the following arguments are required: flow"),
        (["g.npy"], "twoview: g.npy: expected an (H,W,2) or (H,W,3) array, got (6, 9)"),
        (["missing.flo"], "twoview: [Errno 2] No such file or directory: 'missing.flo'"),
        (["f.txt"], "twoview: unsupported flow file: f.txt"),
    )),
    ("run_batch", [], (
        (["--pose", "640"], "error: --pose needs --epipolar"),
        (["--epipolar", "1", "--pose", "0"], "error: --pose needs FOCAL (finite, > 0), got '0'"),
        (["--epipolar", "1", "--pose", "nan"], "error: --pose needs FOCAL (finite, > 0), got 'nan'"),
        (["--epipolar", "1", "--pose", "inf"], "error: --pose needs FOCAL (finite, > 0), got 'inf'"),
        (["--epipolar", "1", "--pose", "x"], "error: --pose needs FOCAL (finite, > 0), got 'x'"),
        (["--epipolar", "1", "--pose"], "error: argument --pose: expected one argument"),
    )),
    ("superpixels", ["i.png", "o.npy"], (
        (["--step", "3"], "error: --step must lie in [4, 64]"),
        (["--step", "65"], "error: --step must lie in [4, 64]"),
        (["--compactness", "-1"], "error: --compactness must lie in [0, 255]"),
        (["--compactness", "256"], "error: --compactness must lie in [0, 255]"),
        (["--iters", "0"], "error: --iters must lie in [1, 32]"),
        (["--iters", "33"], "error: --iters must lie in [1, 32]"),
        (["--min-size", "-1"], "error: --min-size must lie in [0, 67108864]"),
        (["--min-size", "67108865"], "error: --min-size must lie in [0, 67108864]"),
        (["--step", "x"], "error: argument --step: invalid int value: 'x'"),
        (["--boundaries", "b.npy"], "error: --boundaries must be a .png file"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
        (["--flow", "f.flo"], "error: --flow and --fit go together"),
        (["--fit", "o.flo"], "error: --flow and --fit go together"),
        (["--thresh", "1"], "error: --thresh needs --flow and --fit"),
        (["--rounds", "2"], "error: --rounds needs --flow and --fit"),
        (["--classes", "c.png"], "error: --classes needs --flow and --fit"),
        (["--models", "m.npy"], "error: --models needs --flow and --fit"),
        (["--flow", "f.flo", "--fit", "o.png"], "error: --fit must be a .flo or .npy file"),
        (["--flow", "f.flo", "--fit", "o.flo", "--thresh", "0"], "error: --thresh must be finite and > 0"),
        (["--flow", "f.flo", "--fit", "o.flo", "--thresh", "nan"], "error: --thresh must be finite and > 0"),
        (["--flow", "f.flo", "--fit", "o.flo", "--thresh", "inf"], "error: --thresh must be finite and > 0"),
        (["--flow", "f.flo", "--fit", "o.flo", "--rounds", "0"], "error: --rounds must lie in [1, 6]"),
        (["--flow", "f.flo", "--fit", "o.flo", "--rounds", "7"], "error: --rounds must lie in [1, 6]"),
        (["--flow", "f.flo", "--fit", "o.flo", "--classes", "c.npy"], "error: --classes must be a .png file"),
        (["--flow", "f.flo", "--fit", "o.flo", "--models", "m.png"], "error: --models must be a .npy file"),
    )),
    ("superpixels", [], (
        ([], "error: the following arguments are required: image, OUT.npy|OUT.png"),
        (["i.png"], "error: the following arguments are required: OUT.npy|OUT.png"),
        (["i.png", "o.flo"], "error: OUT must be a .npy or .png file"),
    )),
    ("superpixels", [], (
        (["g.npy", "o.npy"], "superpixels: g.npy: not a (H,W,3) uint8 image ((6, 9) float64)"),
        (["missing.png", "o.npy"], "superpixels: [Errno 2] No such file or directory: 'missing.png'"),
        (["i.txt", "o.npy"], "superpixels: i.txt: images are read as .npy, .ppm or .png"),
        (["i.npy", "o.npy", "--flow", "f1.npy", "--fit", "o.flo"], "superpixels: f1.npy is 8x6, i.npy is 9x6"),
        (["i.npy", "o.npy", "--flow", "f.txt", "--fit", "o.flo"], "superpixels: unsupported flow file: f.txt"),
    )),
    ("tracks", [], (
        (["f0.flo"], "error: the following arguments are required: --out"),
        (["--out", "t.npz"], "error: the following arguments are required: FWD.flo"),
        (["f0.flo", "--out", "t.npy"], "error: --out must be a .npz file"),
        (["f0.flo", "f1.flo", "--backward", "b0.flo", "--out", "t.npz"], "error: --backward needs as many files as there are forward flows (2), got 1"),
        (["f0.flo", "--out", "t.npz", "--step", "0"], "error: --step must lie in [1, 256]"),
        (["f0.flo", "--out", "t.npz", "--step", "257"], "error: --step must lie in [1, 256]"),
        (["f0.flo", "--out", "t.npz", "--rel", "nan"], "error: --rel must be finite and >= 0"),
        (["f0.flo", "--out", "t.npz", "--rel", "-1"], "error: --rel must be finite and >= 0"),
        (["f0.flo", "--out", "t.npz", "--abs", "inf"], "error: --abs must be finite and >= 0"),
        (["f0.flo", "--out", "t.npz", "--cap", "0"], "error: --cap must lie in [1, 67108864]"),
        (["f0.flo", "--out", "t.npz", "--cap", "67108865"], "error: --cap must lie in [1, 67108864]"),
        (["f0.flo", "--out", "t.npz", "--flow", "0", "1"], "error: argument --flow: expected 3 arguments"),
        (["f0.flo", "--out", "t.npz", "--flow", "0", "2", "o.flo"], "error: --flow: frames must lie in [0, 1]"),
        (["f0.flo", "--out", "t.npz", "--flow", "-1", "1", "o.flo"], "error: --flow: frames must lie in [0, 1]"),
        (["f0.flo", "--out", "t.npz", "--flow", "a", "1", "o.flo"], "error: --flow needs two frame numbers and a file"),
        (["f0.flo", "--out", "t.npz", "--flow", "0", "1", "o.npy"], "error: --flow: the output must be a .flo file"),
    )),
    ("tracks", [], (
        (["missing.flo", "--out", "t.npz"], "tracks: [Errno 2] No such file or directory: 'missing.flo'"),
        (["f0.txt", "--out", "t.npz"], "tracks: unsupported flow file: f0.txt"),
        (["bad.npy", "--out", "t.npz"], "tracks: bad.npy: expected an (H,W,2) or (H,W,3) array, got (6, 9)"),
        (["f0.npy", "f1.npy", "--out", "t.npz"], "tracks: f1.npy: a 8x6 field among 9x6 ones"),
        (["f0.npy", "--backward", "f1.npy", "--out", "t.npz"], "tracks: f1.npy: a 8x6 field among 9x6 ones"),
    )),
    ("midframe", ["a.png", "b.png", "f.npy", "out.png"], (
        (["--t", "0"], "error: --t must lie in (0, 1)"),
        (["--t", "1"], "error: --t must lie in (0, 1)"),
        (["--t", "nan"], "error: --t must lie in (0, 1)"),
        (["--t", "0.5", "--frames", "2"], "error: --t and --frames exclude each other"),
        (["--frames", "0"], "error: --frames must lie in [1, 99]"),
        (["--frames", "100"], "error: --frames must lie in [1, 99]"),
        (["--fill-rounds", "-1"], "error: --fill-rounds must lie in [0, 64]"),
        (["--fill-rounds", "65"], "error: --fill-rounds must lie in [0, 64]"),
        (["--occl-thresh", "-1"], "error: --occl-thresh must be finite and >= 0"),
        (["--occl-thresh", "inf"], "error: --occl-thresh must be finite and >= 0"),
        (["--occl-thresh", "nan"], "error: --occl-thresh must be finite and >= 0"),
        (["--frames", "2", "--source", "s.png"], "error: --source goes with a single frame, not with --frames"),
        (["--unknown"], "error: unrecognized arguments: --unknown"),
    )),
    ("midframe", [], (
        ([], "error: the following arguments are required: img1, img2, fwd, out"),
        (["a.png", "b.png", "f.npy"], "error: the following arguments are required: out"),
        (["a.png", "b.png", "f.npy", "o.png"], "midframe: the images and the flows differ in size: 8x6, 8x6, 9x6"),
    )),
    ("run_batch", [], (
        (["--mid-fill-rounds", "4"], "error: --mid-fill-rounds and --mid-occl-thresh need --midframe"),
        (["--mid-occl-thresh", "3"], "error: --mid-fill-rounds and --mid-occl-thresh need --midframe"),
        (["--midframe", "--mid-fill-rounds", "65"], "error: --mid-fill-rounds must lie in [0, 64], got 65"),
        (["--midframe", "--mid-fill-rounds", "-1"], "error: --mid-fill-rounds must lie in [0, 64], got -1"),
        (["--midframe", "--mid-occl-thresh", "-1"], "error: --mid-occl-thresh must be finite and >= 0, got -1.0"),
        (["--midframe", "--mid-occl-thresh", "nan"], "error: --mid-occl-thresh must be finite and >= 0, got nan"),
        (["--midframe", "--mid-occl-thresh", "inf"], "error: --mid-occl-thresh must be finite and >= 0, got inf"),
    )),
    ("flowpicture", [], (
        (["f.flo"], "error: nothing to do: give a picture path, --warp, or both"),
        (["f.flo", "--warped", "w.png"], "error: nothing to do: give a picture path, --warp, or both"),
        (["f.npy", "--warp", "a.png", "b.png"], "flowpicture: the flow is 9x6, the images 8x6 and 8x6"),
    )),
    ("spremiZaEpic", ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"], (
        (["--segments"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got []"),
        (["--segments", "20"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20']"),
        (["--segments", "20", "x"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'x']"),
        (["--segments", "2.5", "1"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['2.5', '1']"),
        (["--segments", "-1", "1"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['-1', '1']"),
        (["--segments", "20", "-1"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', '-1']"),
        (["--segments", "20", "nan"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'nan']"),
        (["--segments", "20", "inf"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'inf']"),
        (["--segments", "2147483648", "1"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['2147483648', '1']"),
        (["--segments", "20", "--gpu-epic"], "spremiZaEpic: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', '--gpu-epic']"),
        (["--segments", "20", "1", "--natural-check"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--gpu-epic", "--segments", "20", "1"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--segments", "20", "1", "--segments", "20", "1"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--natural-check", "--gpu-epic", "--prefilter", "--segments", "20", "1"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--segments", "20", "1", "--refine"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
    )),
    ("run_batch", ["--pairs", "1", "--size", "40x48"], (
        (["--segments"], "error: argument --segments: expected 2 arguments"),
        (["--segments", "20"], "error: argument --segments: expected 2 arguments"),
        (["--segments", "20", "x"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'x']"),
        (["--segments", "2.5", "1"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['2.5', '1']"),
        (["--segments", "-1", "1"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['-1', '1']"),
        (["--segments", "20", "-1"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', '-1']"),
        (["--segments", "20", "nan"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'nan']"),
        (["--segments", "20", "inf"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['20', 'inf']"),
        (["--segments", "2147483648", "1"], "error: --segments needs MIN (an integer >= 0) and T (finite, >= 0), got ['2147483648', '1']"),
    )),
    ("python bcd", ["1", "0", "2"], (
        (["--conf-mode", "data"], "error: --conf-mode and --conf-sep need --confidence"),
        (["--conf-sep", "1"], "error: --conf-mode and --conf-sep need --confidence"),
        (["--confidence", "--conf-mode", "chain"], "error: --conf-mode needs M (local or data), got 'chain'"),
        (["--confidence", "--conf-sep", "-1"], "error: --conf-sep needs S (an integer in 0..1024), got '-1'"),
        (["--confidence", "--conf-sep", "1025"], "error: --conf-sep needs S (an integer in 0..1024), got '1025'"),
        (["--confidence", "--conf-sep", "x"], "error: --conf-sep needs S (an integer in 0..1024), got 'x'"),
        (["--confidence", "1"], "error: unrecognized arguments: 1"),
    )),
    ("run_batch", [], (
        (["--confidence"], "error: argument --confidence: expected one argument"),
        (["--confidence", "nan"], "error: --confidence needs T (a number, not NaN), got 'nan'"),
        (["--confidence", "x"], "error: --confidence needs T (a number, not NaN), got 'x'"),
        (["--conf-mode", "data"], "error: --conf-mode and --conf-sep need --confidence"),
        (["--conf-sep", "1"], "error: --conf-mode and --conf-sep need --confidence"),
        (["--confidence", "1", "--conf-mode", "chain"], "error: --conf-mode needs M (local or data), got 'chain'"),
        (["--confidence", "1", "--conf-sep", "1025"], "error: --conf-sep needs S (an integer in 0..1024), got '1025'"),
        (["--confidence", "1", "--conf-sep", "1.5"], "error: --conf-sep needs S (an integer in 0..1024), got '1.5'"),
    )),
    ("spremiZaEpic", ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"], (
        (["--margin"], "spremiZaEpic: --margin needs FILE and T (a number, not NaN), got []"),
        (["--margin", "m.npy"], "spremiZaEpic: --margin needs FILE and T (a number, not NaN), got ['m.npy']"),
        (["--margin", "m.npy", "nan"], "spremiZaEpic: --margin needs FILE and T (a number, not NaN), got ['m.npy', 'nan']"),
        (["--margin", "m.npy", "x"], "spremiZaEpic: --margin needs FILE and T (a number, not NaN), got ['m.npy', 'x']"),
        (["--gpu-epic", "--margin", "m.npy", "1"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--margin", "m.npy", "1", "--segments", "3", "1"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--margin", "m64.npy", "1"], "spremiZaEpic: --margin m64.npy holds float64 (6, 9), expected float32 (6, 9)"),
        (["--margin", "m.npy", "1"], "spremiZaEpic: --margin m.npy holds float32 (6, 8), expected float32 (6, 9)"),
        (["--margin", "missing.npy", "1"], "spremiZaEpic: --margin missing.npy: [Errno 2] No such file or directory: 'missing.npy'"),
    )),
    ("spremiZaEpic", ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"], (
        (["--gpu-epic", "--natural-check"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--natural-check", "--natural-check"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--natural-check", "--refine"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
        (["--gpu-epic", "--prefilter", "--natural-check"], "forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN."),
    )),
    ("spremiZaEpic", [], (
        (["a.png", "b.png", "f.npy", "b.npy", "10", "--natural-check"], "spremiZaEpic: edge kind must be 'canny' or 'sed', not '--natural-check'"),
    )),
    ("daisy i flann", ["3", "0", "1", "--synthetic", "40x48", "--cell", "5x6"], (
        (["--gate", "2"], "error: --gate T needs --pyramid L with L > 1 and a finite T >= 0"),
        (["--pyramid", "1", "--gate", "2"], "error: --gate T needs --pyramid L with L > 1 and a finite T >= 0"),
        (["--pyramid", "2", "--gate", "-1"], "error: --gate T needs --pyramid L with L > 1 and a finite T >= 0"),
        (["--pyramid", "2", "--gate", "nan"], "error: --gate T needs --pyramid L with L > 1 and a finite T >= 0"),
        (["--pyramid", "2", "--gate", "inf"], "error: --gate T needs --pyramid L with L > 1 and a finite T >= 0"),
    )),
)
