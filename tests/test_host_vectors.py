"""The vector sets of host_vectors.py reach what they are meant to reach.  Evaluated from the integer reference alone, on the
CPU: these are requirements on the vectors, not measurements of the code under test.  The bounds asserted here are the table of
DESIGN.md 2.6."""
import digit_vectors as DV
import host_vectors as V
import pymodel_group as PG

P, Q, M51, TOP = V.P, V.Q, V.M51, V.TOP
GROUPS = V.groups()


# ---- F_q ---------------------------------------------------------------------------------------------------------------------
def test_fq_sums_and_differences():
    sums = {a + b for a, b in V.FQ_PAIRS}
    assert {Q - 1, Q, Q + 1, 2 * Q - 2} <= sums
    diffs = {a - b for a, b in V.FQ_PAIRS}
    assert {0, -1, -(Q - 1)} <= diffs
    assert all(a < Q and b < Q for a, b in V.FQ_PAIRS)
    assert {Q - 1, Q, Q + 1, 2 * Q - 2, 2 * Q - 1} <= set(V.FQ_REDUCE_ONCE) and max(V.FQ_REDUCE_ONCE) < 2 * Q


def test_fq_products():
    named = [0, 1, Q - 1, Q - 2, (Q - 1) // 2, 2**252 - 1, 2**252, V.R, V.R2, V.M64, V.M64 << 64, V.M64 << 128]
    pairs = set(V.FQ_MUL_PAIRS)
    assert all((a, b) in pairs for a in named for b in named)
    assert V.M64 << 192 in V.FQ_NONREDUCED and 0x0FFFFFFFFFFFFFFF << 192 in V.FQ_VALUES   # the top limb: all ones is not reduced
    for a in (Q, Q + 1, 2 * Q - 1, 2**256 - 1):
        assert a in V.FQ_NONREDUCED and all((a, b) in pairs for b in named)
    assert all(b < Q for _, b in V.FQ_MUL_PAIRS)
    # what from_bytes_wide multiplies: any 256-bit half by R^2 and by R^3
    assert (2**256 - 1, V.R2) in pairs and (2**256 - 1, V.R3) in pairs
    assert len(GROUPS["fq_mul"].rows) == len(V.FQ_MUL_PAIRS) + 256


def test_fq_mont_reduce_and_conversions():
    assert max(V.FQ_MONT_REDUCE) == Q * 2**256 - 1 and {0, Q, 2**256, (Q - 1) ** 2} <= set(V.FQ_MONT_REDUCE)
    assert {2**512 - 1, (2**256 - 1) << 256, 2**256 - 1} <= set(V.FQ_WIDE)
    kat = V.fq_kat()
    assert V.unwords(int(w, 16) for w in kat["from_bytes_wide_max_raw"]) == (2**512 - 1) % Q
    assert V.unwords(int(w, 16) for w in kat["from_raw_all_ones_equiv_raw"]) == (2**256 - 1) % Q
    assert len(GROUPS["fq_from_bytes_wide"].rows) == len(V.FQ_WIDE) + 2
    assert V.FQ_INVERT[:3] == [0, 1, Q - 1] and {0, 1, V.M64} <= set(V.FQ_U64)
    assert V.words(Q) == [int(w, 16) for w in kat["MODULUS_limbs"]] and V.words(V.R2) == [int(w, 16) for w in kat["R2_limbs"]]


def test_unipoly_and_batch_inversion_values():
    assert {0, 1, Q - 1} <= set(V.poly_values())
    assert sorted({len(b) for b in V.batch_invert_cases()}) == [1, 2, 257]
    assert all(v % Q for b in V.batch_invert_cases() for v in b) and any(Q - 1 in b and 1 in b for b in V.batch_invert_cases())
    for name in ("unipoly_from_evals3", "unipoly_from_evals4", "unipoly_eval3", "unipoly_eval4", "combine_bot3", "host_eq3"):
        assert name in GROUPS


# ---- GF(2^255-19) ------------------------------------------------------------------------------------------------------------
def test_fe_products_reach_the_stated_bound_and_no_further():
    cases = V.fe_mul_cases()
    top, z = [TOP] * 5, [0] * 5
    assert (top, top) in cases
    single = [[TOP if k == i else 0 for k in range(5)] for i in range(5)]
    assert all((a, b) in cases for a in single for b in single) and all((a, top) in cases and (top, a) in cases for a in single)
    assert any(set(a) == {0, TOP} and set(b) == {M51 + 1, TOP} for a, b in cases), "mixed with 0 and 2^51"
    assert all(0 <= x <= TOP for a, b in cases for x in a + b)
    facts = [V.fe_mul_model(a, b) for a, b in cases]
    assert all(f["ok"] for _, f in facts), "a vector wraps a 64- or 128-bit word: it is outside the header's bound"
    # at the bound the carry out of t0 and 19 c out of t4 sit just under 2^64 (field.h: "limbs up to 2^54")
    _, f = V.fe_mul_model(top, top)
    assert 2**63 < f["c0"] < 2**64 and 2**63 < f["c19"] < 2**64
    # ... and one more addition in a lazy chain wraps: the bound is the true one
    assert not V.fe_mul_model([2 * TOP] * 5, [2 * TOP] * 5)[1]["ok"] and not V.fe_mul_model(top, [2 * TOP] * 5)[1]["ok"]
    # what a product returns: limbs 0, 2, 3, 4 below 2^51, limb 1 below 2^51 + 2^13 -- and limb 1 does pass 2^51
    outs = [r for r, _ in facts]
    assert all(V.within(r, V.PROD_MAX) for r in outs) and V.PROD_MAX == [M51, M51 + 2**13, M51, M51, M51]
    assert max(r[1] for r in outs) > M51 + 2**12
    sq = V.fe_square_cases()
    assert tuple(top) in sq and all(tuple(a) in sq for a in single)


def test_fe_subtraction_bias_is_4p_and_the_bound_is_exact():
    assert V.fe_value(V.SUB_BIAS) == 4 * P and V.SUB_BIAS == [4 * (2**51 - 19)] + [4 * (2**51 - 1)] * 4
    z = [0] * 5
    for cases in (V.fe_sub_cases(), V.fe_sub_lazy_cases()):
        assert (z, V.SUB_BIAS) in cases and all((z, [V.SUB_BIAS[k] if k == i else 0 for k in range(5)]) in cases for i in range(5))
        assert not any(V.fe_sub_lazy_model(a, b)[1] for a, b in cases), "a fed vector goes below zero"
    fed = {tuple(r) for name in ("fe_sub", "fe_sub_lazy", "fe_neg", "fe_abs") for r in GROUPS[name].rows}
    above = V.fe_sub_above_cases()
    assert len(above) == 5
    for a, b in above:   # the CPU model alone: a limb goes below zero, the 64-bit word wraps, the field element is wrong
        assert tuple(a + b) not in fed and tuple(b) not in fed
        limbs, under = V.fe_sub_model(a, b)
        assert under and V.fe_value(limbs) % P != (V.fe_value(a) - V.fe_value(b)) % P
        limbs, under = V.fe_sub_lazy_model(a, b)
        assert under and V.fe_value(limbs) % P != (V.fe_value(a) - V.fe_value(b)) % P
    # carried values and product outputs are below the bias (operator-: "for carried inputs"; sub_lazy: "below 2^53")
    assert V.within(V.PROD_MAX, V.SUB_BIAS) and V.within(V.CARRY_MAX, V.SUB_BIAS) and min(V.SUB_BIAS) < 2**53 < min(V.SUB_BIAS) + 80


def test_add_niels_chains_stay_below_2_54():
    worst = 0
    for c in V.niels_cases():
        chain, ok = V.niels_chain_model(*c)
        assert ok
        worst = max([worst] + [x for v in chain.values() for x in v])
    assert 2**53 < worst < 2**54, "E, F, G, H: single lazy sums of product outputs, at their top in the vectors"
    top = list(V.PROD_MAX)
    assert any(p == top * 4 for p, _, _ in V.niels_cases()) and {neg for _, _, neg in V.niels_cases()} == {0, 1}


def test_fe_carry_and_representatives():
    carry = GROUPS["fe_carry"].rows
    assert [2 * m for m in V.PROD_MAX] in carry, "carry on a sum of two product outputs"
    # one pass of carry leaves limb 0 = 2^51 + 18 of this input: why carry() makes two, and a representative of its own below
    src = [M51, M51, M51, M51, 2**51 + M51]
    assert src in carry and V.fe_carry_model(src, passes=1) == [2**51 + 18, M51, M51, M51, M51]
    assert all(V.within(V.fe_carry_model(r), V.CARRY_MAX) for r in carry)
    reps = dict(V.fe_reps())
    vals = {V.fe_value(l) for l in reps.values()}
    assert {P - 1, P, P + 1, 2**255 - 1, 2**255 + 18, 2 * P - 1} <= vals
    assert [2**51 + 18, M51, M51, M51, M51] in reps.values()
    assert {V.fe_value(l) // P for l in reps.values()} >= {0, 1, 2}, "representatives of [0, p), [p, 2p) and above"
    for name in ("fe_to_bytes", "fe_is_negative", "fe_is_zero"):
        assert GROUPS[name].rows == [l for l in reps.values()]
    assert len(GROUPS["fe_equals"].rows) == len(reps) ** 2
    assert any(V.unwords(r) >> 255 for r in GROUPS["fe_from_bytes"].rows), "from_bytes with bit 255 set"
    pw = dict(V.FE_POW_VALUES)
    assert pw["1"] == [1, 0, 0, 0, 0] and V.fe_value(pw["p-1"]) == P - 1 and pw["2"] == [2, 0, 0, 0, 0] and pw["every limb 2^51-1"] == [M51] * 5
    assert GROUPS["fe_invert"].rows == [l for l in pw.values()] == GROUPS["fe_pow_p58"].rows


def test_sqrt_ratio_reaches_its_four_outcomes():
    cases = V.sqrt_ratio_cases()
    outcomes = {V.sqrt_ratio_outcome(u, v) for u, v, _, _ in cases if u and v}
    assert outcomes == {"correct", "flipped", "flipped_i", "none"}
    assert any(u == 0 and v for u, v, _, _ in cases) and any(v == 0 and u for u, v, _, _ in cases) and any(u == 0 == v for u, v, _, _ in cases)
    # a root that would be negative before abs() in some case, so that the sign rule is exercised
    assert any(PG.sqrt_ratio_m1(u, v)[0] and u and v for u, v, _, _ in cases)
    assert any(lu != V.fe_limbs(u) for u, _, lu, _ in cases), "lazy representatives too"
    assert all(V.within(lu, V.SUB_BIAS) for _, _, lu, _ in cases), "u.neg() inside the function takes u up to the bias"


# ---- points ------------------------------------------------------------------------------------------------------------------
def test_torsion_cosets_and_both_rotate_branches():
    ident = PG.Pt.identity()
    for t in V.TORSION4:
        assert (4 * t).X == 0 and (4 * t).Y == (4 * t).Z, "a 4-torsion point"
    assert len({(t.X * pow(t.Z, -1, P) % P, t.Y * pow(t.Z, -1, P) % P) for t in V.TORSION4}) == 4
    for p in [ident] + V.base_points():
        cs = V.coset(p)
        assert len({c.encode() for c in cs}) == 1, "equal bytes"
        if p.X:   # the identity's coset is the torsion itself: x y = 0, nothing to rotate
            assert {V.compress_rotates(c) for c in cs} == {False, True}, "both rotate branches within one coset"
        assert all(a == b for a in cs for b in cs)
        # the second disjunct of equals: X1 Y2 = Y1 X2 fails for half of the pairs of a coset
        assert any((a.X * b.Y - a.Y * b.X) % P for a in cs for b in cs) if p.X else True
        assert p.X == 0 or not (p == -p)
    assert len(GROUPS["pt_compress"].rows) == 2 * 4 * (1 + len(V.base_points())) + 1
    assert ident.encode() == bytes(32) and V.pt_limbs(ident) in GROUPS["pt_compress"].rows, "compress of the identity"
    assert {r[-1] for r in GROUPS["pt_add neg=0"].rows} == {0} and {r[-1] for r in GROUPS["pt_add neg=1"].rows} == {1}
    assert "pt_dbl" in GROUPS and "pt_to_xyzt" in GROUPS and "pt_from_xyzt" in GROUPS
    assert any(p.Z != 1 for p in V.base_points()) and V.gens_point(0).encode() in {p.encode() for p in V.base_points()}


def test_decompress_classes():
    cl = V.decompress_classes()
    assert all(cl.values()), [k for k, v in cl.items() if not v]
    dec = lambda s: PG.decode(s.to_bytes(32, "little"))
    assert cl["identity"] == [0] and dec(0) is not None and dec(0).encode() == bytes(32)
    for name in ("good, x negated", "good, x not negated", "good, small"):
        assert all(dec(s) is not None for s in cl[name]), name
    assert all(V.decode_steps(s)[1] for s in cl["good, x negated"]) and not any(V.decode_steps(s)[1] for s in cl["good, x not negated"])
    assert {P, P + 2, 2**255 - 1} <= set(cl["s >= p"]) and all(P <= s < 2**255 for s in cl["s >= p"])
    # refused by the canonical check ALONE: even, and the value it reduces to would pass the parity test
    assert all(P <= s < 2**255 and s % 2 == 0 for s in cl["s >= p, even"])
    assert all(s >> 255 for s in cl["bit 255 set"]) and any(dec(s & (2**255 - 1)) is not None for s in cl["bit 255 set"])
    # refused by the parity test ALONE: the negative root of a good encoding squares to the same value
    neg = cl["odd s, the negative root of a good one"]
    assert all(s & 1 and s < P and dec(P - s) is not None and all(not x for x in V.decode_steps(s)[2:]) and V.decode_steps(s)[0] for s in neg)
    assert all(s & 1 and s < P for s in cl["odd s"])
    assert cl["s = p - 1 (y = 0)"] == [P - 1] and V.decode_steps(P - 1) == (True, V.decode_steps(P - 1)[1], False, True)
    assert all(s < P and s % 2 == 0 and not V.decode_steps(s)[0] for s in cl["non-square"])
    assert all(V.decode_steps(s)[0] and V.decode_steps(s)[2] and not V.decode_steps(s)[3] for s in cl["negative t"])
    refused = [s for k, v in cl.items() if not k.startswith(("good", "identity")) for s in v]
    assert not any(dec(s) is not None for s in refused)
    assert {s for _, s in V.decompress_all()} == {s for v in cl.values() for s in v}
    assert [V.words(s) for _, s in V.decompress_all()] == GROUPS["pt_decompress"].rows


# ---- wnaf5 -------------------------------------------------------------------------------------------------------------------
def test_wnaf5_vectors_straddle_words_and_ripple():
    cases = dict(V.wnaf5_cases())
    assert {0, 2**253 - 1, Q - 1} <= set(cases.values())
    for w in range(3):
        for b in range(59, 64):
            pos = 64 * w + b
            for span in (1, 2):
                end = min(64 * (w + 1 + span), 252)
                hits = [s for n, s in cases.items() if n.startswith(f"straddle w={w} b={b} ") and n.endswith(f"ones to bit {end}")]
                assert hits, (w, b, span)
                for s in hits:
                    assert s & ((1 << pos) - 1) == 0 and (s >> pos) & 1, "the first set bit is at pos"
                    d = (s >> pos) & 31
                    assert d > 16, "a negative digit: 2^(pos+5) is carried in"
                    assert all((s >> i) & 1 for i in range(pos + 5, end)) and s >> end == 0, "ones above the window up to the word's end"
                    digits, top = V.wnaf5_model(s)
                    assert digits[pos] == d - 32 and top == end and digits[end] == 1, "the carry ripples to the end of the ones"
    # the model itself: the digits sum to the scalar, are odd and at most 15, five apart
    for s in cases.values():
        digits, top = V.wnaf5_model(s)
        assert sum(d << i for i, d in enumerate(digits)) == s
        nz = [i for i, d in enumerate(digits) if d]
        assert all(digits[i] & 1 and abs(digits[i]) <= 15 for i in nz) and all(y - x >= 5 for x, y in zip(nz, nz[1:]))
        assert top == (nz[-1] if nz else -1)
    assert all(s < 2**253 for s in cases.values())


# ---- fixed-base windows and the scalars of the multiplications -----------------------------------------------------------------
def test_fixed_base_window_classes():
    cases = V.fb_cases()
    assert all(s < Q for _, s in cases)
    for w in (0, 1, 13, 24):
        vs = [V.fb_digits(s) for _, s in cases]
        assert any(v[w] == 512 and d[w] == 512 for d, v, _ in vs), f"a tie at 512 in window {w} stays positive"
        assert any(v[w] == 513 and d[w] == -511 for d, v, _ in vs), w
        assert any(v[w] == 1023 and d[w] == -1 for d, v, _ in vs), w
        if w:
            assert any(v[w] == 1024 and d[w] == 0 and v[w + 1] == ((s >> (10 * (w + 1))) & 1023) + 1
                       for (d, v, _), (_, s) in zip(vs, cases)), f"1023 with a carry in: magnitude 0 and a carry out of window {w}"
    assert any(V.fb_digits(s)[1][25] == (s >> 250) + 1 and s >> 250 == top for _, s in cases for top in (0,)), "a carry into the top window"
    assert {s >> 250 for _, s in cases if V.fb_digits(s)[1][25] == (s >> 250) + 1} >= {0, 1, 3}
    # no canonical scalar makes the top window negative or lets a carry leave it
    assert V.fb_digits(Q - 1)[2] == 0 and all(V.fb_digits(s)[2] == 0 and V.fb_digits(s)[0][25] >= 0 for _, s in V.mul_scalars())
    assert all(sum(d << (10 * w) for w, d in enumerate(V.fb_digits(s)[0])) == s for _, s in V.mul_scalars())
    # over the marked table of the harness the two readings of a tie differ
    assert (512 * 1) % Q != (-512 * 1 + 1 * 2) % Q


def test_scalar_sets_of_the_multiplications():
    sc = {s for _, s in V.mul_scalars()}
    assert set(DV.values(10, 26)) <= sc and {s for _, s in V.fb_cases()} <= sc and {0, Q - 1} <= sc
    assert all(s < Q for s in sc)
    assert any(n.startswith("straddle") for n, _ in V.mul_scalars())
    for name in ("pt_mul_bytes B", "pt_mul_bytes gens[0]", "pt_mul_bytes Z!=1", "pt_mul2_bytes", "fb_mul_acc B onto identity",
                 "fb_mul_acc B onto 7B", "fb_mul_acc gens[0] onto identity", "fb_mul_acc gens[0] onto 7B", "fb_mul_acc_marked"):
        assert name in GROUPS and GROUPS[name].rows
    assert len(GROUPS["pt_mul_bytes B"].rows) == len(sc) == len(GROUPS["fb_mul_acc_marked"].rows)
    assert len(GROUPS["fb_mul_acc B onto identity"].rows) == len(sc) + 1   # and zero
    # a generator-stream point: the stream of MultiCommitGens::new, not a multiple of the basepoint anyone knows
    assert V.gens_point(0).encode() != PG.basepoint().encode()


def test_vector_file_round_trip(tmp_path):
    small = {k: GROUPS[k] for k in ("fq_add", "fe_is_zero")}
    path = tmp_path / "v.txt"
    V.write_vector_file(str(path), small)
    text = "".join(f"{g.fn} {len(g.rows)}\n" + "".join(" ".join(f"{w:x}" for w in r[:1]) + "\n" for r in g.rows) for g in small.values())
    assert list(V.parse_output(text, small)) == list(small) and path.read_text().startswith("fq_add ")
