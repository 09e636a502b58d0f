"""average each PMC counter over the dispatches of one kernel (substring match)

    python scripts/pmc_summary.py <root> <kernel substring>                       table on stdout
    python scripts/pmc_summary.py <root> --traffic-json out.json key=substr[,batch,pixels] ...
        HBM traffic record bench.py reads (profiles/rNN_traffic.json): per key the mean FETCH_SIZE / WRITE_SIZE (KiB)
        of the matching dispatches, bytes = 2 * FETCH_SIZE (gfx950: FETCH_SIZE reads half of a wide coalesced
        streaming read, MI355X_MICROARCH.md HBM section) + WRITE_SIZE, the launch shape the record is valid for, and
        a hash of the kernel's source files (bench.py drops the record as stale when they change)
"""
import collections
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHARED = ["s2anet_amd/csrc/mfma_common.hpp", "s2anet_amd/csrc/common.hpp"]
# record key -> (the kernel whose dispatches it averages, the files that kernel is compiled from): an edit of one kernel's
# translation unit leaves the other kernel's record valid
KEYS = {
    "align_conv_pyramid": ("k_dcn_patch", ["s2anet_amd/csrc/dcn_ops.hip"] + _SHARED),
    "conv_tower_pyramid": ("k_conv_f16", ["s2anet_amd/csrc/conv_ops.hip"] + _SHARED),
}


def collect(root, pat):
    agg = collections.defaultdict(list)
    for f in sorted(glob.glob(root + "/p*/*/*_counter_collection.csv") + glob.glob(root + "/p*/*_counter_collection.csv")):
        for r in csv.DictReader(open(f)):
            if pat in r["Kernel_Name"]:
                agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    return agg


def sha16(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(os.path.join(ROOT, p), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def main():
    root = sys.argv[1]
    if sys.argv[2] != "--traffic-json":
        for k, v in collect(root, sys.argv[2]).items():
            print(f"{k:32s} n={len(v):4d} mean={sum(v)/len(v):16.1f} min={min(v):16.1f} max={max(v):16.1f}")
        return
    out, rec = sys.argv[3], {"kernels": {}}
    for spec in sys.argv[4:]:
        key, rest = spec.split("=", 1)
        parts = rest.split(",")
        kernel, sources = KEYS[key]
        assert kernel in parts[0], f"{key} is the record of {kernel}, not of {parts[0]}"
        agg = collect(root, parts[0])
        if not agg.get("FETCH_SIZE") or not agg.get("WRITE_SIZE"):
            print("no FETCH_SIZE / WRITE_SIZE dispatches for", parts[0], file=sys.stderr)
            continue
        fk = sum(agg["FETCH_SIZE"]) / len(agg["FETCH_SIZE"])
        wk = sum(agg["WRITE_SIZE"]) / len(agg["WRITE_SIZE"])
        rec["kernels"][key] = {"kernel": parts[0], "fetch_kib": round(fk, 1), "write_kib": round(wk, 1),
                               "bytes": round((2 * fk + wk) * 1024), "dispatches": len(agg["FETCH_SIZE"]),
                               "batch": int(parts[1]), "pixels": int(parts[2]),
                               "sources": sources, "source_sha16": sha16(sources)}
    rec["command"] = "rocprofv3 --kernel-trace --pmc <FETCH_SIZE | WRITE_SIZE> -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline"
    rec["git_head"] = os.environ.get("S2A_GIT_HEAD")       # filled in when the record is copied into profiles/ (no .git on the GPU box)
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
