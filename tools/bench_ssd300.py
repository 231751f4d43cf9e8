#!/usr/bin/env python3
"""SSD-300 throughput beside SSD-512 (bench.py cannot take a new variant; this is its timing method on the two SSD networks).

  python tools/bench_ssd300.py                  one JSON line: SSD-300 bf16 batch 32 and SSD-512 bf16 batch 16, alternating
  python tools/bench_ssd300.py --ab-pool3       one JSON line: conv3_3 + pool3 (75 -> 38) fused vs conv + stand-alone pool, alternating
  python tools/bench_ssd300.py --layers FILE    the ron_profile_* per-launch table of SSD-300 (one batch in flight)

Timing = bench.py's: parallel.bench_loop, 5 warm-up + 20 timed steps, two batches in flight on two execution slots, a host clock closed
by a synchronise.  Every leg is run --rounds times and reports the median and every round; the legs alternate, their order swaps from
round to round, and only the running leg has a pipeline (second slot + streams), so that no leg's streams share hardware queues with
another's.  The line carries GPU_MAX_HW_QUEUES as the process saw it.
GFLOP / image comes from ron_flops_per_image (2 x MACs over convolutions and heads); peak = 2.5 PFLOP/s dense bf16."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')       # two slots + consumer + default stream (bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0


def make_net(name, dtype, batch, dev, **attrs):
    import torch  # noqa: F401
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network(name)
    net = cls(cls.default_params._replace(num_classes=21), dtype=dtype, max_batch=batch, device=dev, fuse_pools=True)
    for k, v in attrs.items():
        setattr(net, k, v)
    net.load_weights(W.ssd300_synthetic_weights(seed=6) if name == 'ssd_300_vgg' else W.ssd_synthetic_weights(seed=5))
    return net


class Leg(object):
    """One network to time.  Only ONE leg's pipeline (its second execution slot and its streams) exists at a time: with every leg's
    pipeline alive the streams of the later-built ones share hardware queues with the earlier ones' and their two batches in flight
    serialise (pipeline.py warns about it) - the figure would depend on the build order, not on the network."""

    def __init__(self, label, name, dtype, batch, dev, in_flight, **attrs):
        import torch
        from ron_tensorflow_amd import weights as W
        self.label, self.batch, self.in_flight = label, batch, in_flight
        self.net = make_net(name, dtype, batch, dev, **attrs)
        self.images = torch.from_numpy(W.synthetic_images(batch, seed=0, img_shape=self.net.params.img_shape)).to(dev)
        self.ms, self.position = [], []

    def run(self, steps, warmup, dev, position):
        import gc
        import torch
        from ron_tensorflow_amd import parallel
        from ron_tensorflow_amd.pipeline import DetectPipeline
        pipe = DetectPipeline(self.net, slots=self.in_flight, top_k=400)
        res = parallel.bench_loop(pipe, self.images, steps, warmup, self.in_flight, dict(select_threshold=0.01, nms_threshold=0.45),
                                  400, device=dev, check_gather=False, measure_gather=False)
        self.ms.append(res['dt'] / steps * 1e3)
        self.position.append(position)
        det = {f: getattr(res['det'], f).clone() for f in ('count', 'classes', 'scores', 'bboxes', 'anchor_index')}
        torch.cuda.synchronize()
        pipe.close()
        del pipe, res
        gc.collect()
        return det

    def report(self):
        ms = statistics.median(self.ms)
        gflop = self.net.flops_per_image() / 1e9
        ips = self.batch / ms * 1e3
        return dict(images_per_s=ips, ms_per_step=ms, ms_per_step_rounds=[round(m, 4) for m in self.ms], position_in_round=self.position,
                    batch=self.batch,
                    batches_in_flight=self.in_flight, gflop_per_image=gflop, tflops=ips * gflop / 1e3,
                    frac_of_bf16_peak=ips * gflop / 1e3 / PEAK_BF16_TFLOPS, launches=len(self.net.launch_plan()) - 1)

    def close(self):
        self.net.close()


def layer_table(net, images, path, calls=5):
    from ron_tensorflow_amd import _lib
    lib, ctx = _lib.lib(), net._context()
    import torch
    for _ in range(3):
        net.detect(images)
    torch.cuda.synchronize()
    _lib.check(lib.ron_profile_reset(ctx))
    _lib.check(lib.ron_profile_enable(ctx, calls))
    for _ in range(calls):
        net.detect(images)
    torch.cuda.synchronize()
    rows = []
    for i in range(lib.ron_profile_num_ops(ctx)):
        name, conv, fl, ms, n, ab, wb = C.c_char_p(), C.c_int(), C.c_double(), C.c_double(), C.c_int(), C.c_double(), C.c_double()
        _lib.check(lib.ron_profile_get(ctx, i, C.byref(name), C.byref(conv), C.byref(fl), C.byref(ms), C.byref(n), C.byref(ab), C.byref(wb)))
        if n.value:
            us = ms.value / n.value * 1e3
            rows.append((name.value.decode(), us, fl.value * images.shape[0] / (us * 1e-6) / 1e12 if conv.value else 0.0,
                         (ab.value * images.shape[0] + wb.value) / (us * 1e-6) / 1e9))
    with open(path, 'w') as f:
        f.write('# %s batch %d, %d profiled calls, one batch in flight: launch, us, TFLOP/s (convolutions), algorithmic GB/s\n' % (
            type(net).__module__.rsplit('.', 1)[1], images.shape[0], calls))
        for r in rows:
            f.write('%-34s %9.1f %8.1f %8.0f\n' % r)
        f.write('%-34s %9.1f\n' % ('total', sum(r[1] for r in rows)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--in-flight', type=int, default=2)
    ap.add_argument('--ab-pool3', action='store_true', help='SSD-300 with conv3_3 + pool3 fused (the default under fuse_pools) vs conv3_3, '
                    'then the stand-alone pool (RON_CFG_NO_ODD_POOL_FUSE), alternating; checks that the detections are bit-identical')
    ap.add_argument('--only', default='', choices=['', 'ssd300', 'ssd512'], help='time one of the two networks alone (profiler runs)')
    ap.add_argument('--layers', default='', help='write the per-launch table of SSD-300 (and, with --ab-pool3, of the other side) here')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    if args.ab_pool3:
        legs = [Leg('fused_conv3_3+pool3', 'ssd_300_vgg', args.dtype, 32, dev, args.in_flight),
                Leg('conv3_3_then_pool3', 'ssd_300_vgg', args.dtype, 32, dev, args.in_flight, no_odd_pool_fuse=True)]
        assert 'conv3_3+pool3' in legs[0].net.launch_plan() and 'pool3' in legs[1].net.launch_plan()
    else:
        legs = [Leg(label, name, args.dtype, batch, dev, args.in_flight)
                for label, name, batch in (('ssd300', 'ssd_300_vgg', 32), ('ssd512', 'ssd_512_vgg', 16)) if args.only in ('', label)]
    dets = {}
    for r in range(args.rounds):
        # the order of the legs swaps from round to round: a figure that depended on the position would show in ms_per_step_rounds
        for pos, leg in enumerate(legs if r % 2 == 0 else legs[::-1]):
            dets[leg.label] = leg.run(args.steps, args.warmup, dev, pos)
    torch.cuda.synchronize()
    out = dict(tool='bench_ssd300', dtype=args.dtype, steps=args.steps, warmup=args.warmup, rounds=args.rounds, peak_bf16_tflops=PEAK_BF16_TFLOPS,
               gpu_max_hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'))
    for leg in legs:
        out[leg.label] = leg.report()
    if args.ab_pool3:
        a, b = (dets[leg.label] for leg in legs)
        out['bit_identical'] = all(bool(torch.equal(a[f], b[f])) for f in a)
        x = legs[0].images
        pa, pb = (torch.cat([t.reshape(-1) for hs in (leg.net.forward_heads(x)[0], leg.net.forward_heads(x)[2]) for t in hs]) for leg in legs)
        out['heads_bit_identical'] = bool(torch.equal(pa, pb)) and bool(torch.equal(legs[0].net.end_point('pool3', 32), legs[1].net.end_point('pool3', 32)))
        out['fused_over_separate'] = out[legs[0].label]['ms_per_step'] / out[legs[1].label]['ms_per_step']
    if args.layers:
        for k, leg in enumerate(legs if args.ab_pool3 else legs[:2]):
            layer_table(leg.net, leg.images, args.layers if k == 0 else args.layers + '.' + leg.label)
    for leg in legs:
        leg.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
