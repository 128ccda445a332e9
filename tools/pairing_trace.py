"""The BatchNorm pairing in a rocprofv3 kernel trace of bench.py (MMLF_OVERLAP_WGRAD=1):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 3
    python3 tools/pairing_trace.py DIR/*/*_kernel_trace.csv
For every wide weight-gradient launch that another queue's BatchNorm-backward kernels ran beside: its duration and where
those kernels start and end inside it (ms from the weight gradient's start), then the means; the weight-gradient launches
nothing ran beside are summed up as `alone`."""
import csv
import sys


def main(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'], r.get('Queue_Id', '')))
    rows.sort()
    wide = [r for r in rows if 'wgrad4tap_x6w_kernel' in r[2]]
    bn = [r for r in rows if 'bn_reduce_bwd_kernel' in r[2] or 'bn_rows_kernel' in r[2]]
    paired, alone = [], []
    for s, e, _, q in wide:
        beside = [b for b in bn if b[3] != q and b[0] < e and b[1] > s]
        if not beside:
            alone.append((e - s) * 1e-6)
            continue
        rec = {'wgrad_ms': (e - s) * 1e-6}
        for b in beside:
            key = 'reduce' if 'bn_reduce_bwd_kernel' in b[2] else 'apply'
            rec.setdefault(key + '_start', (b[0] - s) * 1e-6)
            rec[key + '_end'] = (b[1] - s) * 1e-6
            rec[key + '_ms'] = rec.get(key + '_ms', 0.0) + (b[1] - b[0]) * 1e-6
        paired.append(rec)
    keys = ['wgrad_ms', 'reduce_start', 'reduce_end', 'reduce_ms', 'apply_start', 'apply_end', 'apply_ms']
    print('# paired wide weight gradients: ms, BatchNorm-backward kernels relative to the weight gradient\'s start')
    print('#', ' '.join(keys))
    for rec in paired:
        print(' '.join(f'{rec.get(k, float("nan")):.3f}' for k in keys))
    if paired:
        print('mean', ' '.join(f'{sum(r.get(k, 0.0) for r in paired) / len(paired):.3f}' for k in keys), f'n={len(paired)}')
    if alone:
        print(f'alone: n={len(alone)} mean {sum(alone) / len(alone):.3f} ms min {min(alone):.3f} max {max(alone):.3f}')


if __name__ == '__main__':
    main(sys.argv[1])
