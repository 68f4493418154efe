"""CPU numerics under which the bit-exact oracle fixtures are taken and checked.

torch's CPU kernels round differently from host to host: Intel MKL picks its code path by CPU vendor, oneDNN and ATen by
instruction set, and reductions split by thread count.  Under this environment (MKL's cross-vendor reproducible path, AVX2
kernels, one thread) the oracle gives the same bits on Intel and AMD hosts.  It must be in place before torch is loaded,
so it is applied to a fresh process (tests/test_cpu_oracle.py) or at the top of a generator script (scripts/gen_golden*.py).
No imports here: a script reads it before importing torch.
"""
PINNED_CPU_ENV = {
    "MKL_CBWR": "COMPATIBLE",
    "MKL_NUM_THREADS": "1",
    "OMP_NUM_THREADS": "1",
    "ATEN_CPU_CAPABILITY": "avx2",
    "ONEDNN_MAX_CPU_ISA": "AVX2",
}
