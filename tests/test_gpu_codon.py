"""GPU: the codon stage (ka_cod_fam; Context.family_codons, kalign_amd.codon) against the numpy restatement
(tests/cod_restate.py) -- records, proteins, stop-free codons and codon rows with np.array_equal / ==, no tolerance -- and
against the goldens recorded from the reference (tests/golden/cod_*.npz): proteins, backtranslated rows and finished codon
alignments.

The pack walks a sequence's raw bytes in steps of 256, four ballots of 64: raw lengths stand at and around 64, 128, 256 and
512, letters at the first and the last byte, a codon's letters on both sides of 63 | 64 and 255 | 256.  The translate takes
64 codons a step: codon counts stand around 64, 128 and 256, stops at lanes 0 and 63 and in a run across 63 | 64.  The
backtranslation walks a row 256 columns a step: widths stand around 64, 256 and 512, gap runs across 255 | 256.  Every
kernel deals four sequences or rows to a workgroup: families of 1 .. 17 sequences put the end of one family and the start
of the next inside one.  The stop-free codon plane has no accessor of its own: a backtranslation copies from it, and every
codon row without its gap bytes is held to the sequence's DNA without stop codons."""
import ctypes as C

import numpy as np
import pytest

import cod_restate as cr
from util import GOLDEN

pytestmark = pytest.mark.gpu

RAW_LENGTHS = [3, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 258, 513]
CODON_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 257]
WIDTHS = [1, 63, 64, 65, 255, 256, 257, 513]
FAMILY_SIZES = [1, 2, 3, 4, 5, 15, 16, 17]
PUNCT, DROP = b"-.*~[`:@!/{", b" \t\n0189\x00\x7f\r"
STOPS = (b"TAA", b"TAG", b"TGA")
G = cr.goldens(GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def params(g=None):
    g = g or G["e2e_fast"]
    return g.subm.reshape(23, 23), g.scal


def codons(rng, n, stops=True):
    """n random codons over A C G T (bytes), the first one ATG; stops=False: none of them a stop"""
    out = [b"ATG"]
    while len(out) < n:
        c = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3))
        if stops or c not in STOPS:
            out.append(c)
    return b"".join(out)


def raw_dna(rng, n, p_gap=0.2, p_drop=0.15, lower=0.3):
    """n raw bytes: letters (some lower case) at the first and the last byte and in between, a multiple of 3 in all, the first
    three A T G; gap characters and dropped bytes between them"""
    kind = rng.random(n)
    letter = kind >= p_gap + p_drop
    letter[[0, -1]] = True
    if n < 6:
        letter[:] = True
    over = int(letter.sum()) % 3
    inner = np.flatnonzero(letter[1:n - 1]) + 1
    if len(inner) >= over:
        letter[rng.permutation(inner)[:over]] = False
    else:
        letter[rng.permutation(np.flatnonzero(~letter))[:3 - over]] = True
    assert letter.sum() % 3 == 0 and letter.sum() >= 3
    a = np.where(kind < p_gap, rng.choice(np.frombuffer(PUNCT, np.uint8), size=n), rng.choice(np.frombuffer(DROP, np.uint8), size=n))
    a[letter] = np.frombuffer(codons(rng, int(letter.sum()) // 3), np.uint8)
    low = letter & (rng.random(n) < lower)
    a[low] |= 32
    return a.astype(np.uint8).tobytes()


def gapped(rng, protein, width, lead=0, trail=0):
    """the protein (bytes) spread over width columns: lead gaps first, trail last, the others at random places"""
    free = width - len(protein) - lead - trail
    assert free >= 0
    where = np.sort(rng.integers(0, len(protein) + 1, size=free))
    row, k = bytearray(b"-" * lead), 0
    for j in range(len(protein) + 1):
        while k < free and where[k] == j:
            row += b"-"
            k += 1
        row += protein[j:j + 1]
    return bytes(row + b"-" * trail)


def check_batch(ctx, fams, rows=None, seed=0):
    """everything one handle says about fams against the restatement -- records, proteins, and, through a backtranslation of
    rows (given, or the proteins spread at random over a width of the family's own), the stop-free codons; returns the
    restatement's dicts and the codon rows"""
    rng = np.random.default_rng(seed)
    want = [[cr.translate(s) for s in f] for f in fams]
    if rows is None:
        rows = []
        for k, f in enumerate(want):
            w = max(len(t["protein"]) for t in f) + (k % 3) * 7
            rows.append([gapped(rng, t["protein"].encode(), w) for t in f])
    cod = ctx.family_codons(fams)
    try:
        seqs, prots = cod.sequences(), cod.proteins()
        cod.back(rows)
        got, prows, st = cod.rows(), cod.protein_rows(), cod.stats()
    finally:
        cod.close()
    assert len(seqs) == len(prots) == len(got) == len(fams)
    for k, f in enumerate(want):
        assert seqs[k].dtype == np.int32 and np.array_equal(seqs[k], [t["rec"] for t in f]), (k, seqs[k].tolist(), [t["rec"] for t in f])
        assert prots[k] == [t["protein"].encode() for t in f], k
        assert prows[k] == list(rows[k]), k
        for i, (s, row, t) in enumerate(zip(fams[k], rows[k], f)):
            assert got[k][i] == cr.backtranslate(row, s).encode(), (k, i)
            assert len(got[k][i]) == 3 * len(row) and got[k][i].replace(b"-", b"") == t["kept"].encode(), (k, i)
    assert (st["launches"], st["syncs"], st["back_launches"], st["back_syncs"]) == (2, 1, 1, 1)
    assert st["bytes"] == sum(len(s) for f in fams for s in f) and st["pack_ms"] > 0.0 and st["translate_ms"] > 0.0 and st["back_ms"] > 0.0
    return want, got


def test_pack_raw_lengths(ctx):
    rng = np.random.default_rng(1)
    fams = [[raw_dna(rng, n) for n in RAW_LENGTHS], [raw_dna(rng, n) for n in reversed(RAW_LENGTHS)],
            [raw_dna(rng, n, p_gap=0.0, p_drop=0.0) for n in RAW_LENGTHS if n % 3 == 0]]
    want, _ = check_batch(ctx, fams)
    assert [t["rec"][0] for t in want[2]] == [n for n in RAW_LENGTHS if n % 3 == 0]
    assert all(t["rec"][1] + t["rec"][2] > 0 for t in want[0][1:])


def test_pack_codons_across_the_ballot_and_the_step_edge(ctx):
    # a codon's three letters on both sides of 63 | 64 and of 255 | 256, in each of its three phases; close together, and
    # with gap characters and dropped bytes between them
    rng = np.random.default_rng(2)
    fam = []
    for edge in (64, 256):
        for phase in range(3):
            start = edge - 1 - phase
            fam.append(b"-" * start + codons(rng, 5))
            fam.append(b"ATG" + b" " * (start - 3) + codons(rng, 4))
            body = codons(rng, 3)
            fam.append(b"." * (start - 2 * phase) + b"- ".join(body[k:k + 1] for k in range(9)) + b"\n")
    want, _ = check_batch(ctx, [fam, fam[::-1]])
    assert [t["rec"][0] for t in want[0]] == [15, 15, 9] * 6


def test_translate_codon_counts_and_stops(ctx):
    rng = np.random.default_rng(3)
    plain = [codons(rng, n) for n in CODON_COUNTS]
    no_stop = [codons(rng, n, stops=False) for n in CODON_COUNTS]
    every = "".join(cr.CODONS).encode()
    body = codons(rng, 200, stops=False)
    cod = [body[3 * k:3 * k + 3] for k in range(200)]
    special = [b"TAA" + body[:3 * 70],                                   # a stop at lane 0
               b"".join(cod[:63] + [b"TGA"] + cod[64:130]),              # ... at lane 63
               b"".join(cod[:127] + [b"TAG"] + cod[128:]),               # ... at lane 63 of the second step
               b"".join(cod[:60] + [STOPS[k % 3] for k in range(9)] + cod[69:150]),      # a run of stops across 63 | 64
               b"TGA" * 256 + b"ATG", b"tag" * 63 + b"gcc", b"TAA" * 64 + b"ATG",       # all but the last codon stops
               every, every.lower(), every[::-1]]
    want, _ = check_batch(ctx, [plain, no_stop, special])
    assert [t["rec"][3] for t in want[0]] == CODON_COUNTS and all(t["rec"][4] == 0 for t in want[1])
    assert [t["rec"][4] for t in want[2][:7]] == [1, 1, 1, 9, 256, 63, 64]
    assert want[2][7]["protein"] == cr.table().decode().replace("*", "") and want[2][7]["rec"][3:] == [64, 3, 0]


def test_translate_goldens(ctx):
    from kalign_amd import codon
    fams, prots = [], []
    for n in sorted(G):
        if n.startswith("translate_"):
            keep = [(s, p) for s, p in zip(G[n].texts("dna"), G[n].texts("protein")) if p]
            fams.append([s for s, _ in keep])
            prots.append([p for _, p in keep])
    out = codon.translate_families(ctx, fams)
    assert [p for p, _ in out] == prots
    x = G["translate_other_letters"]
    k = sorted(n for n in G if n.startswith("translate_")).index("translate_other_letters")
    recs = out[k][1]
    assert recs[:88, 5].tolist() == [1] * 88 and recs[:88, 3].tolist() == [1] * 88 and len(x.texts("dna")) > 88
    check_batch(ctx, fams)


def test_back_widths(ctx):
    rng = np.random.default_rng(4)
    fams, rows = [], []
    for w in WIDTHS:
        lens = sorted({1, max(1, w // 3), max(1, w - 1), w})
        fam = [codons(rng, n, stops=False) + b"TAA" for n in lens]
        prot = [cr.translate(s)["protein"].encode() for s in fam]
        fams.append(fam)
        rows.append([gapped(rng, p, w) if k % 2 else gapped(rng, p, w, lead=(w - len(p)) // 2, trail=(w - len(p)) // 4) for k, p in enumerate(prot)])
    # gap runs across 255 | 256, rows that begin and end in gaps, a row of one residue
    fam = [codons(rng, n, stops=False) for n in (250, 1, 2, 300, 257)]
    prot = [cr.translate(s)["protein"].encode() for s in fam]
    fams.append(fam)
    rows.append([prot[0][:250] + b"-" * 270, b"-" * 255 + prot[1] + b"-" * 264, prot[2][:1] + b"-" * 518 + prot[2][1:],
                 b"-" * 100 + prot[3][:150] + b"-" * 120 + prot[3][150:], prot[4][:255] + b"-" * 263 + prot[4][255:]])
    assert all(len(r) == 520 for r in rows[-1])
    check_batch(ctx, fams, rows)


def test_family_sizes_put_boundaries_inside_workgroups(ctx):
    rng = np.random.default_rng(5)
    fams = [[raw_dna(rng, int(rng.integers(6, 200))) for _ in range(n)] for n in FAMILY_SIZES]
    want, got = check_batch(ctx, fams)
    assert len({len(r[0]) for r in got}) > 4                             # families of different widths
    # the same families in another order put the boundaries elsewhere: every family's results are its own
    _, back = check_batch(ctx, fams[::-1])
    assert [[t["kept"] for t in f] for f in want] == [[r.replace(b"-", b"").decode() for r in f] for f in back[::-1]]


def test_back_goldens(ctx):
    from kalign_amd import codon
    g = G["back_rows"]
    # rows of different widths: a family of one each
    got = codon.backtranslate_families(ctx, [[s] for s in g.texts("dna")], [[r] for r in g.texts("rows")])
    assert got == [[r] for r in g.texts("codon_rows")]
    for n in ("e2e_fast", "e2e_default"):
        g = G[n]
        assert codon.backtranslate_families(ctx, g.families("dna"), g.families("protein_rows")) == g.families("codon_rows")
    assert codon.backtranslate_families(ctx, [[b"ATGTAAGCC", b"gccgcc"]], [["M.A", "AA."]], gap=b".") == [[b"ATG...GCC", b"GCCGCC..."]]


@pytest.mark.parametrize("name", ["e2e_fast", "e2e_default"])
def test_align_codon_families_equals_the_reference(ctx, name):
    from kalign_amd import codon, prepare
    g = G[name]
    fams, kw = g.families("dna"), dict(n_anchors=int(g.n_anchors), weight=float(g.weight))
    rows, prows = codon.align_codon_families(ctx, fams, *params(g), want_protein=True, **kw)
    assert rows == g.families("codon_rows"), name
    assert prows == g.families("protein_rows"), name
    assert prows == prepare.align_families(ctx, g.families("protein"), params(g), biotype=0, **kw)
    for f, (fam, r, p) in enumerate(zip(fams, rows, prows)):
        assert {len(x) for x in r} == {3 * len(p[0])}, f
        for s, x in zip(fam, r):
            assert x.replace(b"-", b"") == cr.translate(s)["kept"].encode()
    assert codon.align_codon_families(ctx, fams, *params(g), **kw) == rows
    assert codon.align_codons(ctx, fams[1], *params(g), **kw) == rows[1]
    assert codon.align_codons(ctx, fams[0], *params(g), want_protein=True, **kw) == (rows[0], prows[0])


def test_a_family_of_one_and_names(ctx):
    from kalign_amd import codon
    g = G["e2e_fast"]
    s = b"atgTAAgc-cN nnTGA"
    rows, prows = codon.align_codon_families(ctx, [[s], g.families("dna")[0]], *params(g), want_protein=True)
    assert rows[0] == [b"ATGGCCNNN"] and prows[0] == [b"MAX"]
    assert rows[1] == g.families("codon_rows")[0]
    # names reach the protein stage's order and leave the rows where the sequences were given
    fam = g.families("dna")[1]
    names = [["s%d" % (len(fam) - k) for k in range(len(fam))]]
    out = codon.align_codon_families(ctx, [fam], *params(g), names=names)
    for x, t in zip(out[0], fam):
        assert x.replace(b"-", b"") == cr.translate(t)["kept"].encode()


def test_mask_by_confidence(ctx):
    from kalign_amd import codon, summary
    g = G["e2e_fast"]
    fams = g.families("codon_rows")[:3]
    rng = np.random.default_rng(6)
    conf = [rng.random(len(f[0]) // 3).astype(np.float32) for f in fams]
    got = codon.mask_by_confidence(ctx, fams, conf, 0.5)
    assert got == summary.mask_by_confidence(ctx, fams, [np.repeat(c, 3) for c in conf], 0.5)
    for (rows, kept), c, f in zip(got, conf, fams):
        assert kept == 3 * int((c.astype(np.float64) >= 0.5).sum()) and len(rows) == len(f) and all(len(r) == kept for r in rows)


def still_aligns(ctx):
    """the context aligns another batch correctly"""
    from kalign_amd import codon
    g = G["e2e_fast"]
    assert codon.align_codon_families(ctx, g.families("dna")[:2], *params(g)) == g.families("codon_rows")[:2]


def test_refusals_name_the_cause(ctx):
    from kalign_amd import KalignAmdError, codon
    ok = [b"ATGGCCTAA", b"atggcc"]
    with pytest.raises(KalignAmdError, match=r"^rc=1: ka_cod_fam_create: family 1, sequence 2: 301 residues, not a multiple of 3$"):
        ctx.family_codons([ok, ok + [b"ATG" * 100 + b"-A", b"AT"], [b"A"]])
    still_aligns(ctx)
    with pytest.raises(KalignAmdError, match=r"^rc=1: ka_cod_fam_create: family 0, sequence 1 has no protein$"):
        ctx.family_codons([[b"ATG", b"TAAtga TAG"], ok])
    with pytest.raises(KalignAmdError, match=r"^rc=1: ka_cod_fam_create: family 1, sequence 0 has no protein$"):
        ctx.family_codons([ok, [b"- 12"]])
    still_aligns(ctx)
    with pytest.raises(KalignAmdError, match=r"^rc=1: ka_cod_fam_create: family 1, sequence 0: byte 0xc3 at offset 5$"):
        ctx.family_codons([ok, [b"ATGGC\xc3\xa9C", b"AT\xffG"], [b"\x80"]])
    still_aligns(ctx)
    with pytest.raises(KalignAmdError, match="one name per sequence"):
        ctx.family_codons([ok], names=[[b"a"]])
    fam = [b"ATGGCCGCCTAAAAA", b"ATG" * 7 + b"TGA"]
    cod = ctx.family_codons([fam])
    try:
        with pytest.raises(KalignAmdError, match=r"^ka_cod_fam_rows_size: nothing has been backtranslated$"):
            cod.rows()
        with pytest.raises(KalignAmdError, match=r"^ka_cod_fam_protein_rows_size: nothing has been backtranslated$"):
            cod.protein_rows()
        with pytest.raises(KalignAmdError, match=r"^rc=1: ka_cod_fam_back: family 0, sequence 1: the row holds 6 residues, the sequence 7 codons without "
                                                 r"stops$"):
            cod.back([[b"MAAK---", b"MMMMMM-"]])
        with pytest.raises(KalignAmdError, match="nothing has been backtranslated"):        # reported before any row is handed out
            cod.rows()
        with pytest.raises(KalignAmdError, match="one protein row per sequence"):
            cod.back([[b"MAAK---"]])
        cod.back([[b"MAAK---", b"MMMMMMM"]])
        want = [[b"ATGGCCGCCAAA" + b"-" * 9, b"ATG" * 7]]
        assert cod.rows() == want
        # a cap one byte short: refused before anything is copied
        need = int(cod.L.ka_cod_fam_rows_size(cod.h))
        assert need == 2 * 22
        buf = np.full(need, 7, np.uint8)
        assert cod.L.ka_cod_fam_rows(cod.h, buf.ctypes.data_as(C.c_void_p), need - 1, None) != 0
        assert cod.L.ka_last_error().decode() == "ka_cod_fam_rows: 43 bytes do not hold the rows (44)" and (buf == 7).all()
        assert cod.L.ka_cod_fam_protein_rows(cod.h, buf.ctypes.data_as(C.c_void_p), 15, None) != 0
        assert cod.L.ka_last_error().decode() == "ka_cod_fam_protein_rows: 15 bytes do not hold the rows (16)" and (buf == 7).all()
        assert cod.rows() == want
    finally:
        cod.close()
    still_aligns(ctx)
    with pytest.raises(KalignAmdError, match=r"ka_cod_fam_back: family 1, sequence 0: the row holds 4 residues, the sequence 3 codons"):
        codon.backtranslate_families(ctx, [[b"ATG"], [b"ATGGCCGCC"]], [[b"M"], [b"MAAA"]])
    still_aligns(ctx)


@pytest.mark.parametrize("n_fam", [1, 40])
def test_launches_and_synchronisations_do_not_grow_with_the_batch(ctx, n_fam):
    rng = np.random.default_rng(7)
    fams = [[codons(rng, int(rng.integers(5, 30))) for _ in range(int(rng.integers(1, 6)))] for _ in range(n_fam)]
    check_batch(ctx, fams)                                               # (2, 1) for create and (1, 1) for the backtranslation
    cod = ctx.family_codons(fams)
    try:
        cod.run(*params())
        st = cod.stats()
        assert (st["launches"], st["syncs"], st["back_launches"], st["back_syncs"]) == (2, 1, 1, 1) and st["run_wall_ms"] > 0.0
        rows = cod.rows()
    finally:
        cod.close()
    for f, r in zip(fams, rows):
        assert [x.replace(b"-", b"") for x in r] == [cr.translate(s)["kept"].encode() for s in f]
