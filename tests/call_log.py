"""The one copy of what the call-sequence tests share: a recorder of the names that go through _lib.call, and the sequences
every pass is made of, at the tests' two sweeps.  A change to a pass's front end is edited in here and nowhere else."""
from conftest import pkg


def record_calls(monkeypatch):
    """From now to the end of the test every _lib.call appends its name to the returned list (and runs as ever)."""
    L = pkg("_lib")
    names, real = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    return names


# DiscreteFlow.front_end without a prior, and what run adds to it with bcd_times=2
FRONT = ["dflow_daisy_pair", "dflow_knn_proposals", "dflow_neighbour_proposals"]
BACK = ["dflow_bcd_prepare", "dflow_bcd_sweep", "dflow_bcd_sweep", "dflow_labels_to_flow"]
# run_batch: the front end of one pass of a group, and `--pairs 1 --bcd-times 2` up to the flows (one group of two passes)
BATCH_PASS = FRONT + ["dflow_bcd_prepare"]
BATCH_FLOWS = 2 * BATCH_PASS + 2 * ["dflow_bcd_sweep_batch"] + 2 * ["dflow_labels_to_flow"]
