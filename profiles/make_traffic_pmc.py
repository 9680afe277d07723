#!/usr/bin/env python3
"""profiles/traffic_pmc.json from the rocprofv3 --pmc passes of tools/r05_pmc_traffic.sh (gpurun_out/r05_prof/pmc_<config>_<counter>):
mean WRITE_SIZE / FETCH_SIZE per launch of the dominant kernel (KiB -> bytes), which bench.py reports as roofline.traffic.
    python profiles/make_traffic_pmc.py gpurun_out/r05_prof r05"""
# A third argument onwards names entries to re-record alone, the others stay:
#     python profiles/make_traffic_pmc.py <directory of the passes> update cfg1
# (cfg1 steps in place since the in-place step: its entry comes from counter-only passes, rocprofv3 --pmc <C> with no tracing in
# the same run, of the bench command with --no-sibling; its scattered 4-byte stores are not the 16-B streaming stores WRITE_SIZE
# is calibrated for, so the figure is what the counter says, not a calibrated byte count.)
import collections, csv, glob, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
src, tag = sys.argv[1], sys.argv[2]
only = sys.argv[3:]
# cfg1: the full-write kernel in the passes of rounds up to r05, the in-place kernel since (whichever the passes hold)
CFG = {"cfg1": (("k_multi<4, 2, false, 2>", "k_step_update<4, 2, false>"), 1048576, 212), "cfg2": ("k_small<5, 2, true, true>", 1048576, 826),
       "cfg4": ("k_lines<false, 16, 2, true, false>", 262144, 2840), "sib4m": ("k_small<4, 2, false, true>", 4194304, 212)}
out = {"_comment": f"HBM traffic per launch from the rocprofv3 PMC passes of round {tag[1:]} (one counter per pass: --pmc WRITE_SIZE / --pmc FETCH_SIZE; units KiB -> bytes x1024), "
                   "command: rocprofv3 --kernel-trace --pmc <C> -- python3 bench.py <config args> --no-cpu-baseline --no-pipelined --no-other-configs --no-entry-points "
                   "--no-learner-side --steps 30 --warmup 5 (tools/r05_pmc_traffic.sh; class defaults: physically contiguous output buffers, static launch policy). gfx950 corrections per "
                   "/opt/skills/guides/MI355X_MICROARCH.md section HBM: WRITE_SIZE is exact for 16-B streaming stores; FETCH_SIZE reads 1/2 of a wide coalesced stream and is "
                   "uncalibrated for narrow loads (the state loads here are 1-4 B per lane), so both the raw and the doubled value are kept and `traffic` uses the doubled one "
                   f"(upper bound). Sources: profiles/{tag}_{{cfg1,cfg2,cfg4,sib4m}}_summary.md."}
if only:  # the other entries and the comment as they are
    out = json.load(open(os.path.join(HERE, "traffic_pmc.json")))
for name, (kernel, boards, bps) in CFG.items():
    if only and name not in only:
        continue
    kernels = [k.replace(" ", "") for k in ((kernel,) if isinstance(kernel, str) else kernel)]
    rec = {"boards": boards, "algorithmic_bytes": boards * bps}
    for counter, key in (("WRITE_SIZE", "write_bytes"), ("FETCH_SIZE", "fetch_bytes_raw")):
        f = glob.glob(os.path.join(src, f"pmc_{name}_{counter}", "**", "*counter_collection.csv"), recursive=True)[0]
        per = collections.defaultdict(list)  # of the names the entry allows, the one the passes launched most often
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter:
                for k, flat in zip((kernel,) if isinstance(kernel, str) else kernel, kernels):
                    if flat in r["Kernel_Name"].replace(" ", ""):
                        per[k].append(float(r["Counter_Value"]))
        rec["kernel"], vals = max(per.items(), key=lambda kv: len(kv[1]))
        rec[key] = int(round(sum(vals) / len(vals) * 1024))
        rec[key.replace("bytes", "launches").replace("_raw", "")] = len(vals)
    rec["fetch_bytes_x2"] = 2 * rec["fetch_bytes_raw"]
    rec["traffic_over_algorithmic"] = round((rec["write_bytes"] + rec["fetch_bytes_x2"]) / rec["algorithmic_bytes"], 4)
    if only:
        rec["passes"] = f"{tag}: counter-only passes (rocprofv3 --pmc, no tracing), algorithmic_bytes is the full-write formula of SURVEY 8d"
    out["cfg1_sibling_4m" if name == "sib4m" else name] = rec
json.dump(out, open(os.path.join(HERE, "traffic_pmc.json"), "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "_comment"}, indent=1))
