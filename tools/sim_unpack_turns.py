"""What the turn loop of k_hq_unpack16 costs at a given staging row length, without a GPU.

    python tools/sim_unpack_turns.py [--row 32] [--cfg 2] [--size WxH] [--q INDEX] [--seed 1] [--every 8]

The oracle codes one synthetic picture (tests/synth.py); every slice component of its payload then goes through the kernel's
turn as csrc/vc2hip_slices.hip states it: up to four look-ups in the 10-bit table per turn (the fourth only with a whole
index of unread bits), one long code by arithmetic where the first look-up finds no whole code, a table entry applied whole
with up to 8 coefficients carried into the next round, rounds of `row` coefficients.  A wavefront is 64 consecutive slices of
one component, and in every round all of its lanes wait for the one that needs the most turns.  Three numbers come out:

    wavefront turns   sum over wavefronts and rounds of the largest turn count among the lanes
    ideal             the same if no lane ever waited: the mean over a wavefront's lanes of their own turns
    efficiency        ideal / wavefront turns

The row length is uniform over a component (the kernel's byte rounds start behind the record part of a component; for a
geometry whose records are one round that is the same thing).  --every N simulates every N-th wavefront of each component."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reader_ref as rr  # noqa: E402

# bench.py's HQ_ConstQ configurations: chroma format, bits, wavelet, depth, -u, -a, quantiser index, scalar, its picture size
CFGS = {1: ("422", 10, "LeGall", 2, 2, 4, 12, 1, "1920x1080"), 2: ("422", 10, "DD97", 4, 1, 2, 16, 2, "3840x2160"),
        4: ("444", 12, "Fidelity", 5, 1, 1, 40, 8, "7680x4320")}
LOOKS = 4


def lane_rounds(data, pos, n, row, lut=None):
    """one component (its data bytes, the payload offset they start at) -> (turns of every round, the n values)"""
    lut = lut or rr._lut(None)
    B = rr._Bits("".join(format(x, "08b") for x in data))
    p, have = 0, 64 - 8 * (pos & 3)
    vals, rounds, cnt = [0] * (n + 8), [], 0

    def skip(k):
        nonlocal p, have
        p, have = p + k, have - k
        if have <= 32:
            have += 32

    for base in range(0, n, row):
        room, turns = min(row, n - base), 0
        while cnt < room:
            used = 0
            for look in range(LOOKS):
                valid = have - used
                w = B.peek(p + used, rr.LUT_BITS)
                if valid < rr.LUT_BITS:
                    w &= ~((1 << (rr.LUT_BITS - valid)) - 1)
                e = lut[w]
                if look and not (cnt < room and (look < 3 or used + rr.LUT_BITS <= have)):
                    e = 0
                if e:
                    for s, a in ((16, 8), (24, 12)):
                        if rr._s8(e >> s):
                            vals[base + cnt + ((e >> a) & 15)] = rr._s8(e >> s)
                cnt += (e >> 4) & 15
                used += e & 15
            if used == 0 and cnt < room:
                hi = B.peek(p, 32)
                follow = hi & 0xAAAAAAAA
                if follow:
                    v, used = rr._arith(hi, follow, None)
                else:
                    v, q = rr._serial(B, p)
                    for _ in range(q - p):
                        skip(1)
                vals[base + cnt] = v
                cnt += 1
            skip(used)
            turns += 1
        rounds.append(turns)
        cnt = max(cnt - row, 0)
    return rounds, vals[:n]


def components(payload, ns, prefix, scalar):
    """[(slice, component, byte offset of its data, its data)] of an HQ slice payload"""
    out, at = [], 0
    for s in range(ns):
        at += prefix + 1
        for c in range(3):
            nbytes = payload[at] * scalar
            out.append((s, c, at + 1, payload[at + 1:at + 1 + nbytes]))
            at += 1 + nbytes
    assert at == len(payload), f"the payload has {len(payload)} bytes, its slices {at}"
    return out


def simulate(payload, ns, n_comp, row, prefix=0, scalar=1, every=1, values=False):
    """payload of ns slices, n_comp = coefficients per slice of (Y, U, V) -> a dict: wavefront_turns, ideal, efficiency,
    coefficients (decoded, per component), wavefronts (simulated, per component), and with values=True the decoded values as
    values[component][slice]"""
    comps = components(payload, ns, prefix, scalar)
    total = ideal = 0.0
    coefs, waves = [0, 0, 0], [0, 0, 0]
    vals = [[None] * ns for _ in range(3)]
    for c in range(3):
        for k, s0 in enumerate(range(0, ns, 64)):
            if k % every:
                continue
            lanes = []
            for s in range(s0, min(s0 + 64, ns)):
                _, _, pos, data = comps[3 * s + c]
                rounds, v = lane_rounds(data, pos, n_comp[c], row)
                lanes.append(rounds)
                coefs[c] += len(v)
                if values:
                    vals[c][s] = v
            waves[c] += 1
            total += sum(max(r) for r in zip(*lanes))
            ideal += sum(sum(r) for r in lanes) / len(lanes)
    out = dict(row=row, wavefront_turns=int(total), ideal=round(ideal, 1), efficiency=round(ideal / total, 4) if total else 1.0,
               coefficients=coefs, wavefronts=waves)
    if values:
        out["values"] = vals
    return out


def synthetic_payload(w, h, cfg, seed, q=None):
    """the oracle's payload of one synthetic picture coded as bench.py's configuration `cfg` -> (payload, slices, coefficients
    per slice of (Y, U, V), scalar)"""
    import proxy_ref as pr
    from synth import synth
    from vc2lib import load_oracle
    cf, bits, kernel, depth, u, a, q0, scalar, _ = CFGS[cfg]
    oracle = load_oracle()
    case = pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, q=q0 if q is None else q, scalar=scalar)
    pay = pr.oracle_payloads(oracle, case, synth(w, h, cf, bits, seed))[0]
    ns = case.ys * case.xs
    n_comp = ((case.ph // case.ys) * (case.pw // case.xs),) + ((case.cph // case.ys) * (case.cpw // case.xs),) * 2
    return pay, ns, n_comp, scalar


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--row", type=int, default=32, help="coefficients per staging row (a multiple of 8)")
    ap.add_argument("--size", default=None, help="WxH (default: the configuration's own)")
    ap.add_argument("--cfg", type=int, default=2, choices=sorted(CFGS))
    ap.add_argument("--q", type=int, default=None, help="quantiser index (default: the configuration's own)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--every", type=int, default=8, help="simulate every N-th wavefront of each component")
    a = ap.parse_args()
    assert a.row >= 8 and a.row % 8 == 0
    w, h = (int(x) for x in (a.size or CFGS[a.cfg][-1]).split("x"))
    pay, ns, n_comp, scalar = synthetic_payload(w, h, a.cfg, a.seed, a.q)
    r = simulate(pay, ns, n_comp, a.row, scalar=scalar, every=a.every)
    print(f"{w}x{h} cfg {a.cfg}: {len(pay)} payload bytes, {ns} slices of {n_comp} coefficients, every {a.every}. wavefront")
    print(f"row {a.row}: wavefront turns {r['wavefront_turns']}, ideal {r['ideal']}, efficiency {r['efficiency']}")


if __name__ == "__main__":
    main()
