"""Times the algebra on POAR tables (ka_ens_merge, ka_ens_select) at one size; prints one JSON line and appends it to
profiles/poar_merge_time.jsonl.

    python tools/poar_merge_time.py --n 512 [--length 300] [--runs 8]

Members: tests/golden/make_golden_ensemble.synthetic, numseq x ~length.  Reported, each named for what it is (HIP events,
the second of two calls, so the kernels are loaded):
  merge_*_device_ms    count and write pass of merge(table of the first half of the members, table of the second half)
  select_*_device_ms   count and write pass of select(first half of the members) on the table of all of them
  table_*_device_ms    for comparison: the existing table pass building the table of all members from their rows
                       (ka_ens_table_write: table_count_ms + table_write_ms)
The operands of merge and select are table-backed (made by select on the device), so no table is built from rows inside the
timed calls.  Up to 512 sequences the results' bytes are also compared with the table of all members / of the first half."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    import kalign_amd
    import make_golden_ensemble as mg

    seqs, members = mg.synthetic(a.n, a.length, a.runs, a.seed, moves=8)
    lens = [len(s) for s in seqs]
    half = a.runs // 2
    ctx = kalign_amd.Context(0)
    out = dict(tool="poar_merge_time", numseq=a.n, length=a.length, runs=a.runs, split=half, residues=sum(lens))

    def handle(rows):
        e = ctx.ensemble(lens, len(rows))
        for k, r in enumerate(rows):
            e.add_member(k, r)
        return e

    whole = handle(members)
    whole.write_table(os.devnull)                            # warm-up: kernels, pinned buffers
    whole.write_table(os.devnull)
    st = whole.stats()
    out["table_count_device_ms"], out["table_write_device_ms"] = st["table_count_ms"], st["table_write_ms"]
    out["table_entries"] = int(st["table_entries"])
    image = whole.table_image() if a.n <= 512 else None      # (beyond that the file is gigabytes: the passes are timed, the bytes not compared)
    # table-backed operands, made on the device: the halves and the whole
    lo, hi, full = whole.select(range(half)), whole.select(range(half, a.runs)), whole.select(range(a.runs))
    for name, make in (("merge", lambda: lo.merge(hi)), ("select", lambda: full.select(range(half)))):
        make().close()                                       # warm-up
        r = make()
        st = r.stats()
        out[name + "_count_device_ms"], out[name + "_write_device_ms"] = st["table_count_ms"], st["table_write_ms"]
        out[name + "_entries"] = int(st["table_entries"])
        if image is not None and name == "merge":
            out["merge_equal_to_table"] = r.table_image() == image
        elif image is not None:
            out["select_equal_to_operand"] = r.table_image() == lo.table_image()
        r.close()
    out["merge_over_table_pass"] = (out["merge_count_device_ms"] + out["merge_write_device_ms"]) / max(
        out["table_count_device_ms"] + out["table_write_device_ms"], 1e-9)
    for e in (full, hi, lo, whole):
        e.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "poar_merge_time.jsonl"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
