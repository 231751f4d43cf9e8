"""Child process of tests/test_ssd300_cpu.py, run with RON_PLAN_ONLY=1 (csrc/common.h: every host-side decision, no HIP call): a
variant-3 context per (dtype, flags, max_batch) is created, fed constant weights and finalised; prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ron_tensorflow_amd import _lib  # noqa: E402


def main():
    assert os.environ.get('RON_PLAN_ONLY') == '1'
    lib = _lib.lib()
    out = []
    for dtype in ('fp32', 'bf16', 'fp16', 'f16x3'):
        for flags in (0, _lib.RON_CFG_FUSE_POOLS):
            for mb in (1, 16, 32):
                cfg = _lib.Config(_lib.VARIANTS['ssd300'], _lib.DTYPES[dtype], 300, 300, 21, mb, 0, flags)
                h = C.c_void_p()
                _lib.check(lib.ron_create(C.byref(h), C.byref(cfg)))
                shapes = []
                for i in range(lib.ron_num_variables(h)):
                    name, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
                    _lib.check(lib.ron_variable_info(h, i, C.byref(name), shape, C.byref(nd)))
                    shp = tuple(shape[k] for k in range(nd.value))
                    shapes.append((name.value.decode(), shp))
                    a = np.full(shp, 1.0 if name.value.endswith(b'gamma') else 0.01, np.float32)
                    _lib.check(lib.ron_load_weight(h, name.value, _lib.ptr(a), (C.c_int64 * 4)(*shp), len(shp)))
                _lib.check(lib.ron_finalize_weights(h))
                hd = _lib.Heads()
                _lib.check(lib.ron_heads_describe(h, C.byref(hd)))
                names = []
                for i in range(lib.ron_profile_num_ops(h)):
                    nm = C.c_char_p()
                    _lib.check(lib.ron_profile_get(h, i, C.byref(nm), None, None, None, None, None, None))
                    names.append(nm.value.decode())
                out.append(dict(dtype=dtype, flags=flags, max_batch=mb, variables=shapes,
                                heads=[(hd.feat_h[i], hd.feat_w[i], hd.num_anchors[i]) for i in range(hd.num_layers)],
                                flops=lib.ron_flops_per_image(h), grouped=lib.ron_num_grouped_launches(h), plan=names))
                _lib.check(lib.ron_destroy(h))
    # the variant accepts 300 x 300 only; variant 7 is still unknown
    for variant, size, want in ((3, 320, b'300 x 300'), (3, 512, b'300 x 300'), (7, 300, b'unknown variant')):
        cfg = _lib.Config(variant, 1, size, size, 21, 1, 0, 0)
        h = C.c_void_p()
        assert lib.ron_create(C.byref(h), C.byref(cfg)) != 0 and want in lib.ron_last_error(), (variant, size, lib.ron_last_error())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
