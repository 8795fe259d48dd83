"""Host side of the BCD statistics (dflow_bcd_stats, DESIGN.md "BCD statistics and the stop rule") that needs no device:
the 48 bytes as a dict, the stop rule, the command-line options of the two drivers and the JSON file they write."""
import json
import math
import struct

STATS_FIELDS = ("smooth_sum", "n_pairs_trunc", "n_data_trunc", "n_changed", "n_bad_label", "data_sum")
STATS_BYTES = 48                      # sizeof(struct dflow_bcd_stats): five uint64 and a double
STOP_KEYS = ("changed_frac", "rel_energy")
HISTORY_ROW = ("sweep",) + STATS_FIELDS + ("energy", "changed_frac")


def stats_dict(buf, lamda, npix):
    """The bytes of one struct dflow_bcd_stats -> a dict of its fields plus energy = lamda * data_sum + smooth_sum (formed here
    in double) and changed_frac = n_changed / npix."""
    if len(buf) != STATS_BYTES:
        raise ValueError("struct dflow_bcd_stats has %d bytes, got %d" % (STATS_BYTES, len(buf)))
    d = dict(zip(STATS_FIELDS, struct.unpack("<5Qd", bytes(buf))))
    d["energy"] = float(lamda) * d["data_sum"] + float(d["smooth_sum"])
    d["changed_frac"] = d["n_changed"] / float(npix)
    return d


def stats_dicts(buf, lamda, npix):
    """The read-back of dflow_bcd_stats_batch, one struct dflow_bcd_stats per pass -> one stats_dict per pass."""
    return [stats_dict(buf[at:at + STATS_BYTES], lamda, npix) for at in range(0, len(buf), STATS_BYTES)]


def check_stop(stop):
    """The stop rule of ceoBCD / ceoBCD_batch: None (fixed sweep count, no statistics), or a dict with changed_frac and / or
    rel_energy (an empty dict: statistics per sweep, no rule).  Returns a plain dict of floats; raises ValueError otherwise."""
    if stop is None:
        return None
    if not isinstance(stop, dict):
        raise ValueError("stop must be None or a dict with %s" % " and / or ".join(STOP_KEYS))
    out = {}
    for k, v in stop.items():
        if k not in STOP_KEYS:
            raise ValueError("stop: unknown key %r (known: %s)" % (k, ", ".join(STOP_KEYS)))
        v = float(v)
        if math.isnan(v):
            raise ValueError("stop[%r] is NaN" % k)
        out[k] = v
    return out


def should_stop(stop, entry, e_prev):
    """Does the sweep whose statistics are `entry` end the pass?  changed_frac: n_changed / (H*W) <= changed_frac.
    rel_energy: (E_prev - E) / E_prev <= rel_energy, E_prev the energy before the sweep, tested as E_prev - E <= rel_energy *
    E_prev so that E_prev = 0 needs no division; a rise of E is a negative left side, so it stops the pass for every
    rel_energy >= 0.  The two forms agree for E_prev > 0, and E >= 0 always: the data costs of used slots lie in [0, tphi]
    (include/dflow.h, dflow_bcd_prepare) and lamda >= 0.  A negative E_prev (costs outside that contract) is refused."""
    if e_prev < 0 or entry["energy"] < 0:
        raise ValueError("the stop rule needs an energy >= 0 (data costs in [0, tphi]); got E_prev = %r, E = %r" % (e_prev, entry["energy"]))
    if "changed_frac" in stop and entry["changed_frac"] <= stop["changed_frac"]:
        return True
    if "rel_energy" in stop and e_prev - entry["energy"] <= stop["rel_energy"] * e_prev:
        return True
    return False


def add_cli_options(ap, stats_flag):
    """--stats / --bcd-stats, --stop-changed F and --stop-energy R of the two drivers."""
    ap.add_argument(stats_flag, dest="bcd_stats", action="store_true",
                    help="report changed labels, data and smoothness sums and the energy E after every sweep; writes bcd_stats.json")
    ap.add_argument("--stop-changed", type=float, default=None, metavar="F",
                    help="end a pass after the sweep that changed at most this fraction of the labels (bcd_times stays the upper bound)")
    ap.add_argument("--stop-energy", type=float, default=None, metavar="R",
                    help="end a pass after the sweep that lowered E by at most this fraction (a rise of E included)")


def stop_from_args(a):
    """The `stop` argument of ceoBCD the options ask for: None when none of the three was given."""
    stop = {}
    if a.stop_changed is not None:
        stop["changed_frac"] = a.stop_changed
    if a.stop_energy is not None:
        stop["rel_energy"] = a.stop_energy
    return stop if (stop or a.bcd_stats) else None


def history_rows(history):
    """A per-sweep history (list of dicts: sweep 0 = the labelling before the first sweep) as JSON rows of HISTORY_ROW."""
    return [{k: h[k] for k in HISTORY_ROW} for h in history]


def history_json(passes, lamda, bcd_times, stop, size):
    """The object bcd_stats.json holds.  passes: list of (name, history)."""
    return {"size": [int(size[0]), int(size[1])], "lamda": float(lamda), "bcd_times": int(bcd_times), "stop": dict(stop or {}),
            "fields": list(HISTORY_ROW),
            "passes": [{"pass": name, "sweeps_run": len(h) - 1, "history": history_rows(h)} for name, h in passes]}


def write_history_json(path, passes, lamda, bcd_times, stop, size, extra=None):
    """extra: further header entries (run_batch.py --pyramid adds "pyramid")."""
    with open(path, "w") as f:
        json.dump(dict(history_json(passes, lamda, bcd_times, stop, size), **(extra or {})), f, indent=1)


def format_row(h):
    """One line per sweep: sweep, changed, data, smooth, E."""
    return "sweep %2d  changed %8d  data %.6f  smooth %d  E %.6f" % (h["sweep"], h["n_changed"], h["data_sum"], h["smooth_sum"], h["energy"])
