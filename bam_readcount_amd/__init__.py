"""bam_readcount_amd — per-position read counts and BasicStat metrics of genome/bam-readcount on the AMD Instinct MI355X.

    capi      ctypes binding of the C-ABI (include/brc.h and the codec / dense-results libraries beside it): engines, regions,
              results as host arrays, text exactly as the reference prints it
    tensors   results of a computed region as arrays where the engine left them: torch tensors on the GPU, filled by the gfx950
              kernels of libbrc_dense_hip.so without a copy through the host (tensors.region); the side libraries beside it, each a
              library and a function of its own: indels, sites (panel), select, bins, runs, vet (the per-allele read-metric
              tests on listed candidates, libbrc_vet_hip.so), vet_indels (the same tests and an allele-aware control veto on
              the records of the indel table, libbrc_ivet_hip.so) and normalize_indels (the indel table left-aligned against
              the reference and its equal records merged, libbrc_inorm_hip.so)
    consensus the binding of the consensus caller (libbrc_cons_hip.so); tensors.consensus is the function over it: a region and its
              indel table turned into a sequence, the per-position calls and the liftover offsets
    shard     splitting a run over ranks / GPUs

Submodules are imported on first use (`from bam_readcount_amd import tensors`); importing the package loads no native library and
needs neither torch nor a GPU.
"""
import importlib

__all__ = ["capi", "tensors", "shard", "consensus"]


def __getattr__(name):
    if name in __all__:
        return importlib.import_module("." + name, __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
