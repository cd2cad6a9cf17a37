#!/usr/bin/env python3
"""Exact arithmetic work of the pairing engine's kernel programs, per item
(one two-pair pairing check), from the generated tables (tools/gen_engine.py):

  product terms  -- one 14 x 14-limb column product each (196 v_mad_u64_u32)
  reductions     -- one Montgomery reduction per output with a product part (196)

summed over the 12 lanes of a group (idle lanes and SIMT padding are not
counted: this is the algorithm's work, not the schedule's).  Writes
profiles/engine_work.json, which bench.py uses for roofline.achieved.

    python tools/engine_work.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_engine as G  # noqa: E402

MADS_PER_PRODUCT = 14 * 14


def program_work(ops, prog):
    by = {op.name: op for op in ops}
    terms = redc = outputs = sub_ops = simt_terms = 0
    for ins in prog:
        if ins[0] != "run":
            continue
        for sub in by[ins[1]].subs:
            sub_ops += 1
            nt = max([len(r.terms) for r in sub] + [0])
            simt_terms += nt + (1 if nt else 0)
            for r in sub:
                terms += len(r.terms)
                outputs += 1
                redc += 1 if r.terms else 0
    return {"product_terms": terms, "reductions": redc, "outputs": outputs, "sub_ops": sub_ops,
            "mads": (terms + redc) * MADS_PER_PRODUCT,
            "simt_lane_mads": 12 * simt_terms * MADS_PER_PRODUCT}


INV_MADS = 32 * 140 + 392  # one field inversion by divsteps (round 4; a^(p-2) was 82 mul + 380 sqr)

MILLER_TAIL_OPS = 7  # miller6_kernels.cuh ENG_MILLER_TAIL_OPS: N1 = Norm(f), the program's last ops


def miller6_work(ops):
    """k_eng_miller6 (miller6.cuh) with its norm tail: six lanes per item, an
    Fp2 product as 3 product terms.  A line product is 3 Fp2 products and 2
    reductions on each lane.  The squaring in the direct form is 3 Fp2
    products on every lane, 2 more terms (the plain square f_i^2) on the even
    lanes, 2 reductions each.  The tail is the 12-lane program's."""
    prog = G.prog_miller()
    n_line = 2 * sum(1 for ins in prog if ins[0] == "ldline")
    n_sqr = sum(1 for ins in prog if ins == ("run", "M_SQR"))
    tail = program_work(ops, prog[-MILLER_TAIL_OPS:])
    assert [ins[1] for ins in prog[-MILLER_TAIL_OPS:]] == ["M_XIF", "M_NRM", "M_XIN2", "M_T012", "M_XIT", "M_D", "M_N1"]
    line_terms, sqr_terms, redc = 6 * 9, 3 * 11 + 3 * 9, 6 * 2
    terms = n_line * line_terms + n_sqr * sqr_terms + tail["product_terms"]
    reductions = (n_line + n_sqr) * redc + tail["reductions"]
    simt = 6 * (n_line * (9 + 2) + n_sqr * (11 + 2)) * MADS_PER_PRODUCT + tail["simt_lane_mads"]
    return {"product_terms": terms, "reductions": reductions, "line_products": n_line, "squarings": n_sqr,
            "tail": tail, "mads": (terms + reductions) * MADS_PER_PRODUCT, "simt_lane_mads": simt}


def feseg6_work(ops, segs):
    """The Karabina FE's segments as shipped: segment 0 on the 12-lane program,
    segments 1..5 in k_eng_fe_seg6 (feseg6.cuh), six lanes per item.  An Fp12
    product (E_MUL, E_MULCJ) is 6 Fp2 products of 3 terms and 2 reductions on
    each lane; a Frobenius map is one Fp2 product by a constant in 4 terms and
    2 reductions on each lane; A <- A^2 is miller6.cuh's general squaring (11
    terms on even lanes, 9 on odd ones, 2 reductions each); conj has no
    products."""
    seg0 = program_work(ops, segs[0])
    runs = [ins[1] for sg in segs[1:] for ins in sg if ins[0] == "run"]
    assert set(runs) <= {"E_XIA", "E_MUL", "E_MULCJ", "E_CONJ", "E_FROB1", "E_FROB2", "E_CYCA"}
    n_mul = sum(1 for r in runs if r in ("E_MUL", "E_MULCJ"))
    n_frob = sum(1 for r in runs if r in ("E_FROB1", "E_FROB2"))
    n_sqr = sum(1 for r in runs if r == "E_CYCA")
    terms = n_mul * 6 * 18 + n_frob * 6 * 4 + n_sqr * (3 * 11 + 3 * 9)
    redc = (n_mul + n_frob + n_sqr) * 6 * 2
    simt = 6 * (n_mul * (18 + 2) + n_frob * (4 + 2) + n_sqr * (11 + 2)) * MADS_PER_PRODUCT
    return {"product_terms": seg0["product_terms"] + terms, "reductions": seg0["reductions"] + redc,
            "fp12_products": n_mul, "frobenius_maps": n_frob, "squarings": n_sqr, "segment0": seg0,
            "mads": seg0["mads"] + (terms + redc) * MADS_PER_PRODUCT,
            "simt_lane_mads": seg0["simt_lane_mads"] + simt}


def main():
    ops = G.build_ops()
    kern = {
        "k_eng_lines": program_work(ops, G.prog_lines()),
        # the shipped Miller kernels (k_eng_miller6 + k_eng_miller_tail); the 12-lane
        # program, which small calls and DGPU_MILLER=lanes12 run, beside it
        "k_eng_miller": miller6_work(ops),
        "k_eng_miller_lanes12": program_work(ops, G.prog_miller()),
        "k_eng_fe": program_work(ops, G.prog_fe()),
        # Montgomery's trick: 3 Fp multiplications per item (392 mads each), one
        # inversion per 64 items amortized (fp.cuh fp_inv: 32 divstep batches of
        # 140 signed 32x32->64 mads, 4,480, plus one multiplication by R^3)
        "k_eng_inv": {"mads": 3 * 392 + INV_MADS // 64},
    }
    # Karabina FE: the 12-lane program segments, the 8-lane
    # compressed chains (63 squarings of the E_CYC records for f1, f2, f4, f5,
    # five exponentiations), and the per-thread decompression side: norms of
    # the six stored values (k_eng_kb_norm: 2 sqr each, 5 mul), their product's
    # inversion (k_eng_inv: 3 mul + an inversion, INV_MADS, per
    # KB_INV_CHAIN items), the per-value inverses and eng_kb_decompress
    # (k_eng_kb_dec: 12 sqr + 5 mul forward, 2 mul + 2 sqr per value after the
    # first backward, 17 mul per decompression)
    segs = G.prog_fe_kb()
    cyc = {o.name: o for o in ops}["E_CYC"].subs[1]
    comp = {G.E_R + c for c in G.KB_COMP}
    sq_terms = sum(len(r.terms) for r in cyc if r.dst in comp)
    sq_redc = sum(1 for r in cyc if r.dst in comp and r.terms)
    n_exp, n_sq = 5, 63
    chain = {"squarings": n_exp * n_sq, "product_terms": n_exp * n_sq * sq_terms,
             "reductions": n_exp * n_sq * sq_redc, "mads": n_exp * n_sq * (sq_terms + sq_redc) * MADS_PER_PRODUCT}
    MUL, SQR = 392, 301
    KB_INV_CHAIN = 16
    ns = len(G.KB_SNAP)
    norm = 2 * ns * SQR + (ns - 1) * MUL
    inv = 3 * MUL + INV_MADS // KB_INV_CHAIN
    dec = 2 * ns * SQR + (ns - 1) * MUL + (ns - 1) * (2 * MUL + 2 * SQR) + ns * 17 * MUL
    # the shipped segment kernels (k_eng_fe_seg(0), then k_eng_fe_seg6); the 12-lane
    # program, which small calls and DGPU_FESEG=lanes12 run, beside it
    seg_work = feseg6_work(ops, segs)
    kern["k_eng_fe_seg"] = seg_work
    kern["k_eng_fe_seg_lanes12"] = program_work(ops, [ins for sg in segs for ins in sg])
    kern["k_eng_kb_chain"] = chain
    kern["k_eng_kb_inv"] = {"mads": n_exp * (norm + inv + dec), "per_exponentiation": {
        "k_eng_kb_norm": norm, "k_eng_inv": inv, "k_eng_kb_dec": dec}}
    kern["k_eng_fe_karabina"] = {"mads": seg_work["mads"] + chain["mads"] + kern["k_eng_kb_inv"]["mads"]}
    # on-G1 schemes: the Miller program with every line formed at its LDLINE
    # from the key's fixed table, 8 of the 12 exports scaled by one Fp
    # multiplication (a P coordinate): 68 line steps x 8 x 392 mads more
    n_ld = sum(1 for ins in G.prog_miller() if ins[0] == "ldline")
    fixed = dict(kern["k_eng_miller_lanes12"])  # k_eng_miller_fixed stays on the 12-lane program
    fixed["line_scalings"] = n_ld * 8
    fixed["mads"] = kern["k_eng_miller_lanes12"]["mads"] + n_ld * 8 * 392
    kern["k_eng_miller_fixed"] = fixed
    out = {
        "unit": "per item (one two-pair pairing check); mads = 32x32->64 v_mad_u64_u32 products the algorithm performs",
        "kernels": kern,
        "pairing_total_mads": sum(kern[k]["mads"] for k in ("k_eng_lines", "k_eng_miller", "k_eng_inv",
                                                             "k_eng_fe_karabina")),
        "pairing_total_mads_granger_scott_fe": sum(kern[k]["mads"] for k in ("k_eng_lines", "k_eng_miller",
                                                                              "k_eng_inv", "k_eng_fe")),
    }
    path = os.path.join(os.path.dirname(HERE), "profiles", "engine_work.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
