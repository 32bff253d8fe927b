"""PMC workload for the quantizer's streaming kernel (tools only; run under rocprofv3 --pmc).

    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU \
        SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM --output-format csv -d <dir> -o a -- python tools/pmc_quant.py
    python tools/pmc_sq_summary.py nf4_quant_blocks_kernel <dir>

32 single-level launches at 4096x4096 (PMC_DTYPE = bf16 / fp16 / fp32, default bf16) over a
rotation of 512 MiB of distinct weights, as tools/bench_quant.py times them.
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nf4_triton_dequantization_amd import _lib  # noqa: E402


def main():
    name = os.environ.get("PMC_DTYPE", "bf16")
    dt, code = {"bf16": (torch.bfloat16, _lib.BF16), "fp16": (torch.float16, _lib.F16),
                "fp32": (torch.float32, _lib.F32)}[name]
    dev = torch.device("cuda", 0)
    numel = 4096 * 4096
    sets = (512 << 20) // (numel * torch.empty((), dtype=dt).element_size())
    ws = [torch.randn(numel, device=dev).to(dt) for _ in range(sets)]
    packed = torch.empty(numel // 2, dtype=torch.uint8, device=dev)
    absmax = torch.empty(numel // 64, dtype=torch.float32, device=dev)
    L = _lib.lib()
    for i in range(32):
        rc = L.nf4_quant_bnb(ws[i % sets].data_ptr(), code, numel, 64, packed.data_ptr(), absmax.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
