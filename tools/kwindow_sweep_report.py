#!/usr/bin/env python3
"""profiles/r29_kwindow_sweep.json from the parity report that tests/conftest.py writes at the end of a GPU session that ran
tests/test_hip_kwindow_random.py:

    python tools/kwindow_sweep_report.py <the session's r06_parity_report.json> profiles/r29_kwindow_sweep.json

Keeps the report's ``kwindow/`` entries and adds, per family (layer / fixed or lengths / lin or log / fp32 or bf16), the worst figure of
each kind and the case that gave it, and the worst per layer over its fp32 families (what DESIGN.md section 6 quotes)."""
import json
import sys

# entry suffix -> (kind, field).  fp32: plain relative errors against the fp64 oracle; bf16 (bits pinned to the scalar layer): the log-mel
# value against the oracle's fp32 value, and lambd.grad against the scalar layer's
KINDS = {"/train/mel": ("out", "plain_max_rel"), "/train/exp_logmel": ("out", "plain_max_rel"), "/no_grad/mel": ("out", "plain_max_rel"),
         "/no_grad/exp_logmel": ("out", "plain_max_rel"), "/dlam": ("dlam", "plain_max_rel"), "/xgrad": ("xgrad", "max_rel"),
         "/logmel_vs_oracle": ("logmel_value_vs_oracle", "plain_max_rel"), "/dlam_vs_scalar": ("dlam_vs_scalar_layer", "max_rel")}


def main(src, dst):
    rep = {k: v for k, v in json.load(open(src)).items() if k.startswith("kwindow/")}
    fam = {}
    for name, st in rep.items():
        _, layer, lens, log, dtype, case, *_ = name.split("/")
        for suffix, (kind, field) in KINDS.items():
            if name.endswith(suffix):
                slot = fam.setdefault("/".join((layer, lens, log, dtype)), {})
                if kind not in slot or st[field] > slot[kind]["worst"]:
                    slot[kind] = {"worst": st[field], "case": case}
    worst = {}
    for key, slot in fam.items():
        layer, _, _, dtype = key.split("/")
        if dtype != "fp32":
            continue
        for kind in ("out", "dlam", "xgrad"):
            if kind in slot and slot[kind]["worst"] >= worst.get(layer, {}).get(kind, {"worst": -1.0})["worst"]:
                worst.setdefault(layer, {})[kind] = dict(slot[kind], family=key)
    zero = sum(st.get("zero_groups", 0) for st in rep.values())
    exempt = sum(st.get("exempt_groups", 0) for st in rep.values())
    out = {"what": "tests/test_hip_kwindow_random.py on the MI355X: the kwindow/ entries of the session's parity report (tests/conftest.py), "
                   "and their maxima.  out, dlam, xgrad: plain relative errors against the fp64 oracle (x.grad: of the largest element, per clip "
                   "with lengths); bf16 families: bits are the scalar layer's by test, the figures are the bf16 log-mel value against the oracle's "
                   "fp32 value and lambd.grad against the scalar layer's.",
           "entries_kept": len(rep), "zero_magnitude_groups": zero, "groups_that_took_the_cancellation_exemption": exempt,
           "worst_per_layer_fp32": worst, "families": dict(sorted(fam.items())), "entries": dict(sorted(rep.items()))}
    with open(dst, "w") as f:
        f.write("{\n")
        for k in list(out)[:-1]:
            f.write(f" {json.dumps(k)}: {json.dumps(out[k], indent=1 if k in ('worst_per_layer_fp32', 'families') else None)},\n")
        f.write(' "entries": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in out["entries"].items()) + "\n }\n}\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
