"""Per-dispatch counters of the block4_cls_pred launch out of a tools/pmc_mfma.sh run: the conv_igemm_kernel dispatches of 200 workgroups
(256 x 224 tile from round 8 on, 256 x 256 before).
    tools/pmc_mfma.sh DIR && python3 tools/pmc_cls_pred.py DIR > cls_pred_counters.json"""
import collections, csv, glob, json, sys
out = sys.argv[1]
rows = collections.defaultdict(dict)
meta = {}
for f in glob.glob('%s/pmc_mfma/*/*counter_collection.csv' % out):
    for r in csv.DictReader(open(f)):
        if 'conv_igemm_kernel' not in r['Kernel_Name'] or 'group' in r['Kernel_Name']:
            continue
        key = (f, r['Dispatch_Id'])
        rows[key][r['Counter_Name']] = rows[key].get(r['Counter_Name'], 0.0) + float(r['Counter_Value'])
        meta[key] = (r['Kernel_Name'], int(r['Grid_Size']), int(r.get('Workgroup_Size', 0) or 0))
sel = {k: v for k, v in rows.items() if meta[k][1] == 200 * 256 and ('256, 224' in meta[k][0] or '256, 256, 2, 2, 2' in meta[k][0])}
names = sorted(set(meta[k][0] for k in sel))
n = len(sel)
tot = collections.defaultdict(float)
for v in sel.values():
    for c, x in v.items():
        tot[c] += x
res = {'kernels': names, 'dispatches': n, 'per_dispatch': {c: x / max(n, 1) for c, x in tot.items()}}
el = tot.get('GRBM_GUI_ACTIVE', 0.0) / 8.0
res['mfma_busy_fraction'] = tot.get('SQ_VALU_MFMA_BUSY_CYCLES', 0.0) / (1024 * el) if el > 0 else None
print(json.dumps(res, indent=1))
