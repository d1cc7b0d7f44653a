"""Local reduce (ftar_reduce_local, LDS variant) on 2 x 256 MiB per launch, rotating over 4 pairs
of buffers (2 GiB: the 256 MiB Infinity Cache holds nothing the next launch reads), one process.
One JSON line per (type, op): TB/s of 3 x 256 MiB per launch (two reads, one write), median and
spread over ROUNDS rounds of LAUNCHES launches each.

    python profiles/int_types/measure.py > profiles/int_types/measure.jsonl
"""
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
spec = importlib.util.spec_from_file_location("ftar_amd", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
ftar = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ftar)

BYTES, PAIRS, LAUNCHES, ROUNDS = 256 << 20, 4, 40, 7
CASES = [("float32", ftar.FLOAT32, ftar.SUM, 4), ("bfloat16", ftar.BFLOAT16, ftar.SUM, 2), ("uint8", ftar.UINT8, ftar.SUM, 1),
         ("uint8", ftar.UINT8, ftar.MAX, 1), ("int16", ftar.INT16, ftar.PROD, 2), ("uint64", ftar.UINT64, ftar.MAX, 8),
         ("uint8", ftar.UINT8, ftar.PROD, 1), ("uint8", ftar.UINT8, ftar.LAND, 1), ("int8", ftar.INT8, ftar.MAX, 1),
         ("uint16", ftar.UINT16, ftar.LAND, 2), ("bfloat16", ftar.BFLOAT16, ftar.MAX, 2), ("float32", ftar.FLOAT32, ftar.SUM, 4)]
OPS = {ftar.SUM: "SUM", ftar.PROD: "PROD", ftar.MAX: "MAX", ftar.LAND: "LAND"}


def main():
    dev = torch.device("cuda:0")
    ftar.set_reduce_variant(1)
    g = torch.Generator(device=dev).manual_seed(1)
    # byte patterns with the top nibble clear: finite, normal-range values as float32 / bfloat16 too
    bufs = [(torch.randint(0, 64, (BYTES,), dtype=torch.uint8, device=dev, generator=g),
             torch.randint(0, 64, (BYTES,), dtype=torch.uint8, device=dev, generator=g)) for _ in range(PAIRS)]
    for name, dt, op, es in CASES:
        n = BYTES // es
        rates = []
        for r in range(ROUNDS + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(LAUNCHES):
                x, y = bufs[k % PAIRS]
                ftar.reduce_local(x, y, count=n, dtype=dt, op=op)
            b.record()
            torch.cuda.synchronize()
            if r:  # round 0 warms up
                rates.append(3.0 * BYTES * LAUNCHES / (a.elapsed_time(b) * 1e-3) / 1e12)
        print(json.dumps({"type": name, "op": OPS[op], "bytes_per_operand": BYTES, "launches": LAUNCHES,
                          "tb_per_s_median": round(statistics.median(rates), 3), "tb_per_s_min": round(min(rates), 3),
                          "tb_per_s_max": round(max(rates), 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
