#!/usr/bin/env python3
"""Distribution of wave-tile start/end times inside one temporally blocked pass (GPU box)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import effectivediffusivityfvm_amd as pkg  # noqa: E402
from effectivediffusivityfvm_amd import _capi  # noqa: E402

CHAIN = "--chain" in sys.argv                                       # chained passes in one launch (k_sweep_matfree_tb_chain)
sys.argv = [a for a in sys.argv if a != "--chain"]
# --deep FIRST PASSES: stamp passes FIRST ... FIRST + 2 of a chain of PASSES (default 60 of 150: the steady state of bench.py's
# launch); --deep 0 3 is the start of a chain
FIRST, PASSES = 60, 150
if "--deep" in sys.argv:
    k = sys.argv.index("--deep")
    FIRST, PASSES = int(sys.argv[k + 1]), int(sys.argv[k + 2])
    del sys.argv[k:k + 3]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 0
with pkg.Solver(n, n) as s:
    if T:
        s.set_tuning("tb_T", T)
    for k, v in zip(("tb_rank_w0", "tb_rank_w1", "tb_rank_w2", "tb_rank_wall"), sys.argv[3:7]):
        s.set_tuning(k, int(v))
    if os.environ.get("TB_RANKED") is not None:
        s.set_tuning("tb_ranked", int(os.environ["TB_RANKED"]))
    try:
        s.set_tuning("tb_chain", 1 if CHAIN else 0)                 # (one pass per launch unless asked: the stamps below are of ONE pass)
    except Exception:
        assert not CHAIN                                            # an older build of the library (DEFF_AMD_LIB): no such key, never chained
    s.synth_image(12345, 0)
    s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
    s.init_linear(0.0, 1.0)
    s.sweeps(48)
    if CHAIN:
        s.sweeps(3 * 8 * PASSES)                                    # (the clocks of an idle chip: a chain right after start-up ran a fifth slower)
    L = _capi.load()
    nt = C.c_int()
    _capi.check(L.deff_debug_tb_stamps(s._ctx, 2.0 / 3.0, None, C.byref(nt)))
    buf = np.zeros(2 * nt.value, dtype=np.uint64)
    if CHAIN:
        buf[0], buf[1] = FIRST, PASSES                               # the header: first pass to stamp, passes of the chain
    _capi.check(L.deff_debug_tb_stamps(s._ctx, 2.0 / 3.0, buf.ctypes.data_as(C.c_void_p), C.byref(nt)))
    if CHAIN:
        # two header words, then 20 words per tile: entry, where it ran, then for three passes {neighbours seen, first row
        # consumed, steady-state loop entered, swept (last store issued), stores acknowledged, flag published}
        assert s.plan_value("tb_chain") == 1 and s.plan_value("tb_fallbacks") == 0, "the plan is not chained"
        w = buf[2:].reshape(-1, 20)
        w = w[w[:, 0] > 0].astype(np.int64)
        t0 = w[:, 0].min()
        ev = (w[:, 2:].reshape(len(w), 3, 6) - t0) / 100.0          # [tile, pass, event] in us
        seen, first, steady, swept, acked, pub = (ev[:, :, k] for k in range(6))
        simd = w[:, 1] >> 4
        print(f"n={n} tiles={len(w)} chained launch of {PASSES} passes, stamped {FIRST}...{FIRST + 2}; pass {FIRST} starts at {seen[:, 0].min():.1f} us")
        period = np.concatenate([seen[:, 1] - seen[:, 0], seen[:, 2] - seen[:, 1]])
        print(f"  (a) period (a tile's start of a pass to its start of the next): mean {period.mean():.2f} p5 {np.percentile(period, 5):.2f} p50 {np.median(period):.2f} p95 {np.percentile(period, 95):.2f}")
        sweep = swept - seen                                        # the whole of tb_strip
        own = pub[:, :2] - swept[:, :2]                             # stores acknowledged + flag
        wait = seen[:, 1:] - pub[:, :2]                             # list (unless it came with the acknowledgement) + polls + waiting
        parts = (("first row (request -> consumed)", first - seen), ("ramp (first row -> steady loop)", steady - first),
                 ("steady loop", swept - steady), ("sweep = the three", sweep), ("stores acknowledged", acked[:, :2] - swept[:, :2]),
                 ("flag", pub[:, :2] - acked[:, :2]), ("until neighbours seen", wait))
        for name, v in parts:
            print(f"      {name:32s} mean {v.mean():6.2f} p5 {np.percentile(v, 5):6.2f} p50 {np.median(v):6.2f} p95 {np.percentile(v, 95):6.2f} max {v.max():6.2f}")
        print(f"      sum of the means: sweep {sweep.mean():.2f} + own (acknowledged, flag) {own.mean():.2f} + until seen {wait.mean():.2f} = {sweep.mean() + own.mean() + wait.mean():.2f}")
        # (b) the slowest tiles: is their own path what the period consists of?
        slow = np.argsort(sweep.mean(axis=1))[::-1][:max(len(w) // 20, 1)]
        ws, os_, ss = wait[slow], own[slow], sweep[slow]
        print(f"  (b) slowest 5 % of tiles by sweep time ({len(slow)}): sweep mean {ss.mean():.2f} min {ss.min():.2f}; own mean {os_.mean():.2f}; until neighbours seen mean {ws.mean():.2f} p50 {np.median(ws):.2f} p95 {np.percentile(ws, 95):.2f} max {ws.max():.2f}")
        print(f"      their first row {(first - seen)[slow].mean():.2f}, ramp {(steady - first)[slow].mean():.2f}, steady loop {(swept - steady)[slow].mean():.2f}; sweep + own + until seen = {ss.mean() + os_.mean() + ws.mean():.2f} against the period {period.mean():.2f}")
        fast = np.argsort(sweep.mean(axis=1))[:max(len(w) // 20, 1)]
        print(f"      fastest 5 %: sweep mean {sweep[fast].mean():.2f}; until neighbours seen mean {wait[fast].mean():.2f}")
        last = np.array([swept[simd == k, 2].max() for k in np.unique(simd)])
        print(f"  a SIMD's last wave ends pass {FIRST + 2}: mean {last.mean():.1f} min {last.min():.1f} max {last.max():.1f}")
        sys.exit(0)
    st = buf[0::2].astype(np.int64)
    dur_t = (buf[1::2] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    where = (buf[1::2] >> np.uint64(32)).astype(np.int64)          # HW_ID[15:0] | XCC << 16
    ok = dur_t > 0
    t0 = st[ok].min()
    st, dur, where = (st[ok] - t0) / 100.0, dur_t[ok] / 100.0, where[ok]   # microseconds
    en = st + dur
    print(f"n={n} tiles={ok.sum()} launch span {en.max():.1f} us")
    for name, v in (("start", st), ("end", en), ("duration", dur)):
        q = np.percentile(v, [0, 5, 25, 50, 75, 95, 100])
        print(f"  {name:9s} min {q[0]:7.1f}  p5 {q[1]:7.1f}  p25 {q[2]:7.1f}  p50 {q[3]:7.1f}  p75 {q[4]:7.1f}  p95 {q[5]:7.1f}  max {q[6]:7.1f}")
    print(f"  mean duration / span = {dur.mean() / en.max():.3f}")
    # per SIMD (XCC, SE, CU, SIMD of HW_ID): when its waves end, oldest first
    simd = where >> 4                                              # drop the wave slot
    ids = np.unique(simd)
    ends = {k: np.sort(en[simd == k]) for k in ids}
    cnt = np.array([len(v) for v in ends.values()])
    last = np.array([v[-1] for v in ends.values()])
    print(f"  SIMDs seen {len(ids)}; waves per SIMD: " + ", ".join(f"{c} x{(cnt == c).sum()}" for c in np.unique(cnt)))
    for k in range(cnt.max()):
        v = np.array([e[k] for e in ends.values() if len(e) > k])
        print(f"  end of a SIMD's wave #{k + 1}: mean {v.mean():6.1f}  p5 {np.percentile(v, 5):6.1f}  p95 {np.percentile(v, 95):6.1f}")
    print(f"  a SIMD's last wave ends: mean {last.mean():.1f}  min {last.min():.1f}  max {last.max():.1f} us -> SIMD-time idle before the launch ends: {1 - last.mean() / en.max():.3f}")
    # does the wave slot (HW_ID[3:0]) tell the order in which a SIMD serves its waves?
    from collections import Counter
    order = Counter()
    for k in ids:
        m = simd == k
        order[tuple((where[m] & 15)[np.argsort(en[m])].tolist())] += 1
    print("  wave slots of a SIMD in the order its waves end: " + ", ".join(f"{k} x{v}" for k, v in order.most_common(8)))
    # ... and does the workgroup's index tell the slot?  (blockIdx = kk * 8 + xcd, workgroup tile bt = xcd * per + kk, 4 waves each)
    wt_all = np.nonzero(ok)[0]
    nbt = (nt.value + 3) // 4
    per = (nbt + 7) // 8
    kk = (wt_all // 4) % per
    slot = where & 15
    for sl in np.unique(slot):
        v = kk[slot == sl]
        print(f"  wave slot {sl}: workgroups kk (position in its XCD's dispatch order) min {v.min()} p5 {int(np.percentile(v, 5))} median {int(np.median(v))} p95 {int(np.percentile(v, 95))} max {v.max()}")
    # the stragglers: which tiles end last?
    plan = s.plan()
    gy = plan["tb_chunks_per_image"]
    late = np.argsort(en)[::-1][:24]
    if plan.get("tb_ranked"):                                       # dealt tiles: index = rank * strips * nq + tx * nq + q
        nq = plan["tb_chunks_per_image"] // 3
        per_cls = plan["tb_strips"] * nq
        print(f"  dealt tiles, {nq} chunks per rank and strip; last 24: " + "  ".join(f"[rank {wt_all[i] // per_cls} tx {(wt_all[i] % per_cls) // nq} q {wt_all[i] % nq} slot {where[i] & 15}: {en[i]:.1f}]" for i in late))
        for c in range(3):
            mm = wt_all // per_cls == c
            print(f"  rank {c}: {mm.sum()} tiles, end mean {en[mm].mean():.1f} p95 {np.percentile(en[mm], 95):.1f} max {en[mm].max():.1f}; slots " + str(sorted(set((where[mm] & 15).tolist()))))
        print("  the same with where they ran: " + "  ".join(f"[r{wt_all[i] // per_cls} tx{(wt_all[i] % per_cls) // nq} q{wt_all[i] % nq} xcc{where[i] >> 16} se{(where[i] >> 13) & 7} cu{(where[i] >> 8) & 15} simd{(where[i] >> 4) & 3}: {en[i]:.1f}]" for i in np.argsort(en)[::-1][:48]))
        cu_id = where >> 6                                         # XCC, SE, CU (drop SIMD and slot)
        cu_end = {k: en[cu_id == k].max() for k in np.unique(cu_id)}
        ce = np.array(sorted(cu_end.values()))
        print(f"  CUs {len(ce)}: last end of a CU p5 {np.percentile(ce, 5):.1f} median {np.median(ce):.1f} p95 {np.percentile(ce, 95):.1f} max {ce.max():.1f}; the 8 slowest: " + " ".join(f"{v:.1f}" for v in ce[-8:]))
        txd = (wt_all % per_cls) // nq
        print("  mean end by strip: " + " ".join(f"{t}:{en[txd == t].mean():.0f}" for t in np.unique(txd)))
        sys.exit(0)
    ntx_ = plan["tb_strips"]                                        # equal chunks, default numbering (tb_xmajor = 1): wt = chunk * strips + strip
    print("  last 24 tiles to end: " + "  ".join(f"[tx {wt_all[i] % ntx_} ch {wt_all[i] // ntx_} xcc {where[i] >> 16} cu {(where[i] >> 8) & 15} se {(where[i] >> 13) & 7} simd {(where[i] >> 4) & 3} slot {where[i] & 15}: {en[i]:.1f}]" for i in late))
    txs = wt_all % ntx_
    for name, m in (("first strip", txs == 0), ("last strip", txs == txs.max()), ("inner strips", (txs > 0) & (txs < txs.max()))):
        for sl in (0, 1, 2):
            mm = m & (slot == sl)
            if mm.any():
                print(f"  {name:12s} slot {sl}: {mm.sum():4d} tiles, duration mean {dur[mm].mean():6.1f} max {dur[mm].max():6.1f}")
    xcc = where >> 16
    for xc in np.unique(xcc):
        m = xcc == xc
        print(f"  XCC {xc}: tiles {m.sum():4d}  last end {en[m].max():6.1f}  mean end {en[m].mean():6.1f}")
