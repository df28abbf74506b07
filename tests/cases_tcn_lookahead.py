"""Geometries and the runner of the fixed-latency streaming tests (test_tcn_lookahead_cpu.py, test_tcn_lookahead_gpu.py):
data only.  Builders, `walk` and the schedules a / b / c are those of cases_tcn_stream."""
import torch

import cases_tcn_stream as cs

# H, blocks, K, FiLM: one geometry per channel-tile instantiation NT = ceil(H / 16) of the convolution kernel; K odd
GEOMETRIES = {1: (1, 1, 3, False), 16: (16, 3, 15, True), 24: (24, 3, 5, False), 48: (48, 3, 15, True), 64: (64, 2, 7, False),
              72: (72, 3, 15, True), 96: (96, 2, 9, True), 100: (100, 3, 15, False), 128: (128, 2, 15, True)}

# clip lengths around the latency 98 of (16, 3, 15), and the pieces flush() drains in
SHORT_T = (1, 2, 97, 98, 99, 196, 197)
FLUSH_BLOCKS = (1, 64, 4096)


def case(H, nb, K, film, B=2, T=1100, causal=False):
    return cs.case(H, nb, K, film, B=B, T=T, causal=causal)


def latency(c):
    return 0 if c["causal"] else (c["K"] - 1) * (2 ** c["nb"] - 1)


def run(stream, x, sizes):
    """The pushes of x cut into `sizes` and the flush, without the first `latency` samples: the whole-clip result."""
    out, t = [], 0
    for n in sizes:
        y = stream.push(x[:, :, t:t + n])
        assert y.shape == (x.shape[0], 8, n)
        out.append(y)
        t += n
    assert t == x.shape[2]
    tail = stream.flush()
    assert tail.shape == (x.shape[0], 8, stream.latency)
    return torch.cat(out + [tail], 2)[:, :, stream.latency:]
