"""CPU-side checks of mast3r_slam_backends as a package of per-header modules
(no GPU needed): every wrapper reaches the library through the package's
``_lib`` at call time, so a swapped library (the test build, a variant) is the
one they all call; every symbol is declared once, in its module's SIGNATURES
table, which is what ``_load`` applies and what the *_EXPORTS lists are."""
import pytest


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


class Recorder:
    """Stands in for the library: notes every symbol asked for, then forwards."""

    def __init__(self, lib):
        self.lib, self.seen = lib, []

    def __getattr__(self, symbol):
        self.seen.append(symbol)
        return getattr(self.lib, symbol)


# one device-free call per module that has one (rope, attn and head have none)
DEVICE_FREE = [
    ("gn", "m3s_version", lambda be: be.version()),
    ("gn", "m3s_gn_layout_debug", lambda be: be.workspace_layout(3, 16, 2)),
    ("match", "m3s_match_dense_workspace_size", lambda be: be.match_dense_workspace_size(1, 4, 4)),
    ("gn", "m3s_track_workspace_size", lambda be: be.track_workspace_size(16)),
    ("gn", "m3s_track_frame_workspace_size", lambda be: be.track_frame_workspace_size(16)),
    ("retrieval", "m3s_asmk_store_size", lambda be: be.asmk_store_size(4, 16, 32)),
    ("retrieval", "m3s_asmk_quantize_workspace_size", lambda be: be.asmk_quantize_workspace_size(4, 8, 2)),
]


def test_every_module_calls_the_swapped_library(be):
    real = be._lib
    rec = Recorder(real)
    be._lib = rec
    try:
        for _, symbol, call in DEVICE_FREE:
            before = len(rec.seen)
            assert call(be)
            assert rec.seen[before:] == [symbol], symbol
    finally:
        be._lib = real
    assert be._lib is real
    before = len(rec.seen)
    be.version()
    assert len(rec.seen) == before  # restored: the stand-in is left alone


def tables(be):
    return [m._SIGNATURES for m in be._MODULES]


def test_every_table_symbol_gets_its_signature_on_load(be):
    lib = be._load()  # a fresh handle: nothing set by an earlier load
    assert lib is not be._lib
    n = 0
    for table in tables(be):
        for symbol, (restype, argtypes) in table.items():
            fn = getattr(lib, symbol)
            assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), symbol
            assert fn.restype is restype, symbol
            n += 1
    assert n == sum(len(t) for t in tables(be)) > 0


def test_tables_are_the_export_lists(be):
    union = [s for t in tables(be) for s in t]
    assert len(union) == len(set(union))  # no symbol in two tables
    exports = [be.EXPORTS, be.RETRIEVAL_EXPORTS, be.ROPE_EXPORTS, be.ATTN_EXPORTS, be.HEAD_EXPORTS]
    assert set(union) == set().union(*exports)
    assert len(union) == sum(len(e) for e in exports)
