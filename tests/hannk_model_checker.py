"""The evaluator of halide_amd.hannk_model's plans: walks model.setup and model.plan on numpy arrays.  Generator steps go through the plain-C
checkers of the same name (hannk_checker, hannk_nn_checker, hannk_program_checker: three modules over one object); fill, copy_from and gather are numpy (as_strided views and
np.take).  Independent of the HIP code; of the package it reads the plan and nothing else."""
import numpy as np

import hannk_checker as hk
import hannk_nn_checker as hn
import hannk_program_checker as hp


class Evaluator:
    def __init__(self, model):
        self.model = model
        self.mem = {}
        for i, t in enumerate(model.tensors):
            if t.alias is None:
                n = max(int(np.prod(t.shape, dtype=np.int64)), 1)
                self.mem[i] = np.zeros(n, t.dtype) if t.data is None else np.ascontiguousarray(t.data, t.dtype).reshape(-1).copy()
        for s in model.setup:
            self.step(s)

    def flat(self, i):
        a = self.model.tensors[i].alias
        return self.mem[i if a is None else a]

    def view(self, v):
        flat = self.flat(v.tensor)
        it = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[v.offset:], tuple(v.extents[::-1]), tuple(s * it for s in v.strides[::-1]))

    def run(self, *inputs):
        m = self.model
        acts = [i for i in m.graph.inputs if m.graph.tensors[i].data is None]
        assert len(acts) == len(inputs)
        for i, x in zip(acts, inputs):
            self.flat(i)[...] = np.ascontiguousarray(x, m.tensors[i].dtype).reshape(-1)
        for s in m.plan:
            self.step(s)
        return [self.flat(i).reshape(tuple(reversed(m.tensors[i].shape))).copy() for i in m.graph.outputs]

    def step(self, s):
        a = s.args
        V = self.view
        n = s.name
        if n == "tile_conv_filter_uint8":
            V(a[3])[...] = hk.tile_filter(V(a[0]), a[1], a[2], a[3].extents)
        elif n == "conv_u8_u8_u8":
            V(a[14])[...] = hk.conv(V(a[0]), V(a[2]), V(a[4]), a[14].extents, (a[5], a[6]), (a[7], a[8]), a[1], a[3], a[9], a[10], a[11], a[12], a[13],
                                    in_mins=a[0].mins, out_mins=a[14].mins)
        elif n in ("depthwise_conv_uint8", "depthwise_conv_broadcast_uint8"):
            assert a[9] == 0
            V(a[15])[...] = hk.depthwise(V(a[0]), V(a[2]), V(a[4]), a[15].extents, (a[5], a[6]), (a[7], a[8]), a[1], a[3], a[10], a[11], a[12], a[13], a[14],
                                         broadcast=n.endswith("broadcast_uint8"), in_mins=a[0].mins, out_mins=a[15].mins)
        elif n == "fill_uint8":
            V(a[1])[...] = np.uint8(a[0])
        elif n == "copy_uint8_uint8":
            V(a[2])[...] = hp.copy(V(a[0]), a[2].extents, a[1], a[0].mins, a[2].mins)
        elif n == "upsample_channels_uint8":
            V(a[2])[...] = hp.upsample_channels(V(a[0]), a[1], a[2].extents, a[0].mins, a[2].mins)
        elif n in ("average_pool_uint8", "max_pool_uint8"):
            V(a[7])[...] = hn.pool("average" if n.startswith("average") else "max", V(a[0]), a[7].extents, (a[1], a[2]), (a[3], a[4]), a[5], a[6], a[0].mins,
                                   a[7].mins)
        elif n == "mean_uint8":
            V(a[9])[...] = hn.mean(V(a[0]), a[9].extents, a[1:9:2], a[2:9:2], a[0].mins, a[9].mins)
        elif n == "add_uint8_uint8":
            V(a[9])[...] = hn.add(V(a[0]), a[1], a[2], V(a[3]), a[4], a[5], a[6], a[7], a[8], a[9].extents)
        elif n == "mul_uint8_uint8_uint8":
            V(a[9])[...] = hn.mul(V(a[0]), a[1], V(a[2]), a[3], a[4], a[5], a[6], a[7], a[8], a[9].extents)
        elif n == "softmax_uint8":
            V(a[6])[...] = hn.softmax(V(a[0]), a[1], a[2], a[3], a[4], a[5], a[6].extents)
        elif n == "l2_normalization_uint8":
            V(a[2])[...] = hn.l2_normalization(V(a[0]), a[1], a[2].extents)
        elif n == "elementwise_5xuint8_1xuint8":
            V(a[6])[...] = hp.elementwise([V(x) for x in a[:5]], V(a[5]))
        elif n == "hannk_copy_from":
            assert a[0].mins == a[1].mins and a[0].extents == a[1].extents      # the lowering builds views of one box
            V(a[1])[...] = V(a[0])
        elif n == "hannk_gather":
            src, idx, dst = V(a[0]), V(a[1]), V(a[3])
            dst[...] = np.take(src, idx, src.ndim - 1 - a[2])
        else:
            raise AssertionError(f"no checker for step {n}")
