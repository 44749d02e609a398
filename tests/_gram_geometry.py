"""Test-side restatement of the Gram launch geometry (csrc/pca_eig.h pca_gram_ksplit, csrc/pca.hip
gram_kernel), shared by test_hip_pca_batches.py and test_lines.py."""
import re


def num_cu_of(ctx):
    m = re.search(r"(\d+) CUs", ctx.name)
    return int(m.group(1)) if m else 256


def gram_geometry(num_cu, ntiles, Nz):
    """(ksplit, zper) as gram_launch / gram_kernel (csrc/pca.hip) pick them."""
    ksplit = max(1, min(32, (num_cu * 8 + ntiles - 1) // ntiles))
    if ksplit > Nz // 64:
        ksplit = max(Nz // 64, 1)
    zper = ((Nz + ksplit - 1) // ksplit + 3) & ~3
    return ksplit, zper
