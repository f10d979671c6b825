"""aindex_amd — MI355X-native k-mer counting and perfect-hash lookup engine.

Drop-in for the count_kmers / compute_index / compute_aindex / batch get_tf_values path of
ad3002/aindex: same `AindexWrapper` / `AIndex` Python API and the same on-disk `.pf`, `.tf.bin`,
`.kmers.bin`, `.index.bin`, `.indices.bin` layouts; the work runs in hand-written HIP kernels for
gfx950 behind the C ABI declared in include/aindex_hip.h.
"""
__version__ = "0.1.0"


_ANALYSIS = ("iter_reads_by_kmer", "iter_reads_by_sequence", "get_srandness")


def __getattr__(name):
    # the analysis functions of aindex.py, importable from the package as from the reference's; resolved on first use, so that importing
    # the package alone (and `import *`) still loads nothing
    if name in _ANALYSIS:
        from . import aindex
        return getattr(aindex, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
