"""Times the ensemble's POAR table (ka_ens_table_*, ka_ens_open_table) at one size; prints one JSON line and appends it to
profiles/poar_table_time.jsonl.

    python tools/poar_table_time.py --n 512 [--length 300] [--runs 8] [--ref]

Members: tests/golden/make_golden_ensemble.synthetic, numseq x ~length.  Reported, each named for what it is:
  *_device_ms   HIP events: the table's count and write passes; score, confidence and the per-level candidate passes
                of consensus(min_support=1) on the member-backed handle and, in the same process, on a handle opened from
                the table the first one wrote
  *_wall_ms     host wall time: write_table to a file, ensemble_from_table from that file
  ref_*_ms      with --ref and oracle/_ref built: the reference's extract_poars loop + poar_table_write, and poar_table_read,
                on one thread of this machine
The greedy union is the same host code behind both handles and dominates consensus(): its time is reported once per
handle, for completeness, not compared."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def stage(e, seqs, members, tag, out):
    """score of every member, confidence of member 0, consensus(min_support=1): device ms of each on handle e"""
    e.score(members[0])                                      # warms up the kernels (and builds the maps)
    ms = []
    for rows in members:
        e.score(rows)
        ms.append(e.stats()["score_ms"])
    out[tag + "_member_score_device_ms"] = ms
    e.confidence(members[0])
    e.confidence(members[0])
    out[tag + "_confidence_device_ms"] = e.stats()["confidence_ms"]
    cons = e.consensus(seqs, 1)
    st = e.stats()
    out[tag + "_level_candidates"] = st["level_candidates"]
    out[tag + "_level_device_ms"] = {L: round(v, 3) for L, v in st["level_ms"].items()}
    out[tag + "_count_device_ms"], out[tag + "_write_device_ms"] = st["count_ms"], st["write_ms"]
    out[tag + "_greedy_host_ms"] = st["greedy_host_ms"]
    return cons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ref", action="store_true", help="also time the reference's table, its write and its read")
    a = ap.parse_args()

    import kalign_amd
    import make_golden_ensemble as mg

    seqs, members = mg.synthetic(a.n, a.length, a.runs, a.seed, moves=8)
    lens = [len(s) for s in seqs]
    ctx = kalign_amd.Context(0)
    out = dict(tool="poar_table_time", numseq=a.n, length=a.length, runs=a.runs, residues=sum(lens))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.poar")
        m = ctx.ensemble(lens, a.runs)
        for k, rows in enumerate(members):
            m.add_member(k, rows)
        m.score(members[0])                                  # the maps
        m.write_table(path)                                  # warm-up: kernels, pinned buffers, the file
        t0 = time.perf_counter()
        m.write_table(path)
        out["write_table_wall_ms"] = (time.perf_counter() - t0) * 1e3
        st = m.stats()
        for k in ("table_count_ms", "table_write_ms"):
            out[k.replace("_ms", "_device_ms")] = st[k]
        out["table_host_write_ms"], out["table_wait_host_ms"] = st["table_host_ms"], st["table_wait_host_ms"]
        out["table_entries"], out["table_chunks"] = int(st["table_entries"]), int(st["table_chunks"])
        out["table_bytes"] = os.path.getsize(path)
        t0 = time.perf_counter()
        t = ctx.ensemble_from_table(lens, path=path)
        out["ensemble_from_table_wall_ms"] = (time.perf_counter() - t0) * 1e3
        out["table_host_read_check_upload_ms"] = t.stats()["table_host_ms"]
        cm = stage(m, seqs, members, "members", out)
        ct = stage(t, seqs, members, "table", out)
        out["consensus_equal"] = cm == ct
        out["table_passes_over_one_level"] = (out["table_count_device_ms"] + out["table_write_device_ms"]) / max(
            max(out["members_level_device_ms"].values()), 1e-9)
        t.close()
        m.close()
        ctx.close()
        if a.ref:
            if not mg.available():
                out["ref"] = "not measured: oracle/_ref not built"
            else:
                import make_golden_poar as mp
                L = mp.lib()
                t0 = time.perf_counter()
                tab = mg.Table(members)
                t1 = time.perf_counter()
                rp = os.path.join(d, "r.poar")
                assert L.poar_table_write(tab.t, rp.encode()) == 0
                t2 = time.perf_counter()
                tab.close()
                t3 = time.perf_counter()
                mp.reference_read(rp)
                t4 = time.perf_counter()
                out["ref_extract_poars_ms"], out["ref_poar_table_write_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
                out["ref_poar_table_read_ms"] = (t4 - t3) * 1e3
                out["table_equal_to_ref"] = open(rp, "rb").read() == open(path, "rb").read()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "poar_table_time.jsonl"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
