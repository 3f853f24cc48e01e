"""Where the Q1 preparation runs, from a rocprofv3 --kernel-trace CSV of scripts/time_eigh.py (LAST decomposition of the trace):
  * the tail of the band reduction (panels with a trailing size <= TAIL_NT): span, union of the busy intervals, idle share, the
    kernel time weighted with the share of the 256 CUs a launch can cover (one workgroup per CU), and
    the factorisation chain's time per panel (first to last kernel of the panel's chain on the look-ahead stream);
  * the Q1 stage: the preparation issued in line (end of Q2 .. end of the last V T image) and the rest;
  * how many reflector blocks (ot_extract_v_kernel launches) were prepared inside the band reduction.
Prints one JSON object.  usage: trace_q1_tail.py <kernel_trace.csv> <n> [TAIL_NT = 8192]"""
import csv, json, statistics, sys

SB = 64
CUS = 256


def union_ns(ivs):
    ivs = sorted(ivs)
    if not ivs:
        return 0
    tot, (cs, ce) = 0, ivs[0]
    for s, e in ivs[1:]:
        if s > ce:
            tot += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    return tot + ce - cs


def main():
    path, n = sys.argv[1], int(sys.argv[2])
    tail_nt = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
    rows = list(csv.DictReader(open(path)))
    skey = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
    for r in rows:
        r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        r["k"] = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("jx::", "")
        r["q"] = r.get(skey, "")
        wg = 1
        for ax in "XYZ":
            wg *= max(1, int(r["Grid_Size_" + ax]) // max(1, int(r["Workgroup_Size_" + ax])))
        r["wgs"] = wg
    rows.sort(key=lambda r: r["s"])
    ext = [i for i, r in enumerate(rows) if r["k"].startswith("sb_extract_band_kernel")]
    lo = ext[-2] + 1 if len(ext) > 1 else 0
    dec = rows[lo:]                                   # the last decomposition (and whatever the script ran after it)
    i_ext = ext[-1] - lo
    i_chol = next(i for i, r in enumerate(dec) if r["k"].startswith("sb_chol_kernel"))
    band = dec[max(i_chol - 1, 0):i_ext]              # from the first panel's Gram product on
    recon = [i for i, r in enumerate(band) if r["k"].startswith("sb_recon_kernel")]
    npan = len(recon)
    p0 = next(p for p in range(npan) if n - SB * p - SB <= tail_nt)    # first panel of the tail
    t0, t1 = band[recon[p0]]["e"], dec[i_ext]["s"]
    seg = [r for r in band if r["s"] >= t0]
    is_prep = lambda r: r["k"].startswith(("ot_", "oz_"))
    busy = union_ns((r["s"], min(r["e"], t1)) for r in seg)
    busy_noprep = union_ns((r["s"], min(r["e"], t1)) for r in seg if not is_prep(r))
    # chains: kernels of the look-ahead stream, cut behind every sb_copy_v_kernel
    side = band[recon[min(p0, npan - 1)]]["q"] if npan > 1 else None
    chains, cur = [], []
    for r in band:
        if r["q"] != side or is_prep(r):
            continue
        cur.append(r)
        if r["k"].startswith("sb_copy_v_kernel"):
            chains.append(cur)
            cur = []
    tail_chains = [c for c in chains if c[0]["s"] >= t0]
    ch_ms = [(c[-1]["e"] - c[0]["s"]) / 1e6 for c in tail_chains]
    out = {
        "n": n, "tail_nt": tail_nt, "stream_key": skey, "panels": npan, "tail_panels": npan - p0,
        "tail_span_ms": (t1 - t0) / 1e6, "tail_busy_union_ms": busy / 1e6, "tail_idle_share": 1.0 - busy / (t1 - t0),
        "tail_busy_union_without_preparation_ms": busy_noprep / 1e6,
        "tail_kernel_time_sum_ms": sum(r["e"] - r["s"] for r in seg) / 1e6,
        # kernel time weighted with the share of the CUs its grid can cover: what a full chip would have needed
        "tail_cu_weighted_time_ms": sum((r["e"] - r["s"]) * min(1.0, r["wgs"] / CUS) for r in seg) / 1e6,
        "tail_time_in_launches_below_a_quarter_of_the_cus_ms": union_ns((r["s"], min(r["e"], t1)) for r in seg if r["wgs"] * 4 <= CUS) / 1e6,
        "tail_time_with_a_launch_above_three_quarters_of_the_cus_ms": union_ns((r["s"], min(r["e"], t1)) for r in seg if r["wgs"] * 4 > 3 * CUS) / 1e6,
        "tail_chain_ms_per_panel_mean": statistics.mean(ch_ms) if ch_ms else None,
        "tail_chain_ms_per_panel_median": statistics.median(ch_ms) if ch_ms else None,
        "tail_chains": len(ch_ms),
        "band_span_ms": (t1 - band[0]["s"]) / 1e6,
        "blocks_prepared_inside_band_reduction": sum(r["k"].startswith("ot_extract_v_kernel") for r in band),
    }
    prep_in_band = [r for r in band if is_prep(r)]
    if prep_in_band:
        out["preparation_in_band_kernel_time_sum_ms"] = sum(r["e"] - r["s"] for r in prep_in_band) / 1e6
        out["preparation_in_band_first_to_last_ms"] = (prep_in_band[-1]["e"] - prep_in_band[0]["s"]) / 1e6
        out["preparation_in_band_ends_before_band_end_ms"] = (t1 - prep_in_band[-1]["e"]) / 1e6
    # Q1 stage: behind the last Q2 kernel
    post = dec[i_ext:]
    q2 = [i for i, r in enumerate(post) if "sbback_apply" in r["k"]]
    if q2:
        q1 = post[q2[-1] + 1:]
        q1 = [r for r in q1 if r["k"].startswith(("ot_", "oz_", "dg_")) or "Memset" in r["k"] or "fill" in r["k"].lower()]
        q2_end = post[q2[-1]]["e"]
        dg = [i for i, r in enumerate(q1) if r["k"].startswith("dg_")]
        prep_end = q2_end
        if dg:
            nxt = next((r for r in q1[dg[-1]:] if r["k"].startswith("oz_slice_kernel")), None)
            prep_end = nxt["e"] if nxt else q1[dg[-1]]["e"]
        last_mm = [r for r in q1 if r["k"].startswith("oz_mm_kernel")]
        q1_end = last_mm[-1]["e"] if last_mm else q1[-1]["e"]
        out["q1_span_ms"] = (q1_end - q2_end) / 1e6
        out["q1_preparation_in_line_ms"] = (prep_end - q2_end) / 1e6
        out["q1_blocks_prepared_in_line"] = sum(r["k"].startswith("ot_extract_v_kernel") for r in q1)
    print(json.dumps(out, indent=1))


main()
