"""bench.py against an alternative libdflow.so (tools/prof_build/<name>): python tools/bench_variant.py <lib> [--no-daisy-pair] [bench args]
--no-daisy-pair: for a library built before dflow_daisy_pair existed; load_pair then makes two dflow_daisy calls, as it did then."""
import sys, os, importlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
_lib = importlib.import_module("lk-s-2022-estimacija-pokreta_amd._lib")
_lib.LIB_PATH = os.path.join(ROOT, "tools", "prof_build", sys.argv[1])
args = sys.argv[2:]
if "--no-daisy-pair" in args:
    args.remove("--no-daisy-pair")
    del _lib._SIGNATURES["dflow_daisy_pair"]
    DF = importlib.import_module("lk-s-2022-estimacija-pokreta_amd.pipeline").DiscreteFlow
    DF.load_pair = lambda self, a, b: (self.izracunajDaisy(a, out=self.descrs1), self.izracunajDaisy(b, out=self.descrs2)) and None
sys.argv = ["bench.py"] + args
import bench
bench.main()
