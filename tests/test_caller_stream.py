"""Completeness of the caller's-stream tests (tests/test_caller_stream_gpu.py): every function include/kdlae.h
declares with a `void* stream` parameter is a case of that file's table or a key of its EXEMPT dict, never both, and
neither names anything the header does not declare.  Runs without a GPU: the table builds its calls lazily."""
import os
import re

from tests import test_caller_stream_gpu as G

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kdlae.h")


def _declarations():
    """name -> parameter list of every function the header declares (comments and struct bodies removed)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = text.replace('extern "C" {', " ")                # its closing brace stays behind, alone
    while True:                                             # struct and enum bodies, innermost first
        stripped = re.sub(r"\{[^{}]*\}", " ", text)
        if stripped == text:
            break
        text = stripped
    decls = {}
    for m in re.finditer(r"\b([A-Za-z_]\w*)\s*\(([^()]*)\)\s*;", text):
        assert m.group(1) not in decls, m.group(1)
        decls[m.group(1)] = " ".join(m.group(2).split())
    return decls


def _takes_stream(params):
    return re.search(r"\bvoid\s*\*\s*stream\b", params) is not None


def test_the_parser_sees_the_header():
    decls = _declarations()
    assert len(decls) > 100
    assert _takes_stream(decls["kdlae_t_forward"]) and _takes_stream(decls["kdlae_train_mask_frames"])
    assert _takes_stream(decls["kdlae_data_sample"]) and _takes_stream(decls["kdlae_debug_infer"])
    assert not _takes_stream(decls["kdlae_tt_mark_sync"]) and not _takes_stream(decls["kdlae_tile_plan"])


def test_every_entry_with_a_stream_is_a_case_or_exempt():
    decls = _declarations()
    with_stream = {name for name, params in decls.items() if _takes_stream(params)}
    cases, exempt = G.covered(), set(G.EXEMPT)
    assert not cases - with_stream, f"cases for entries without a stream parameter: {sorted(cases - with_stream)}"
    assert not exempt - set(decls), f"EXEMPT names what the header does not declare: {sorted(exempt - set(decls))}"
    assert not cases & exempt, f"both a case and exempt: {sorted(cases & exempt)}"
    missing = with_stream - cases - exempt
    assert not missing, f"entries that take a stream and are neither a case nor exempt: {sorted(missing)}"
    # an exempt entry without a stream parameter is there because it waits, allocates or reads host memory
    for name in exempt - with_stream:
        assert re.search(r"_(set_param|prepare|mark_sync|create|create_restormer|destroy)$", name), name


# what the lines an exemption cites must say, by entry (one phrase per cited range, in order; an edit that moves the
# header's lines shows up here as a citation that no longer points at its sentence)
PHRASES = {
    "_commit_params": ["synchronous"],
    "_set_param": ["HOST memory"],
    "_prepare": ["kdlae_t_prepare"],
    "kdlae_t_prepare": ["synchronous copy"],
    "kdlae_tt_mark_sync": ["kdlae_tt_mark_sync waits on the host"],
    "kdlae_data_sample": ["may wait on the host"],
    "kdlae_t_debug_sr_fold": ["test_sr_fold_gpu"],
    "_create": ["neither waits on"], "_create_restormer": ["neither waits on"], "_destroy": ["neither waits on"],
    "kdlae_debug_": ["self-test entry points"],
}


def _phrases(name):
    if name in PHRASES:
        return PHRASES[name]
    hits = [v for k, v in PHRASES.items() if (k.startswith("_") and name.endswith(k)) or
            (k.endswith("_") and name.startswith(k))]
    assert len(hits) == 1, name
    return hits[0]


def test_every_exemption_cites_lines_that_say_so():
    lines = open(HEADER).read().splitlines()
    for name, reason in G.EXEMPT.items():
        cited = re.findall(r"kdlae\.h:(\d+)(?:-(\d+))?", reason)
        assert cited, (name, reason)
        text = " ".join(" ".join(lines[int(lo) - 1:int(hi or lo)]) for lo, hi in cited)
        for phrase in _phrases(name):
            assert phrase in text, f"{name}: the lines its reason cites ({reason}) do not say '{phrase}'"


def test_the_table_is_well_formed():
    ids = [c[0] for c in G.CASES]
    assert len(ids) == len(set(ids))
    for cid, names, factory, checks, debug in G.CASES:
        assert names and callable(factory) and checks and set(checks) <= {G.S12, G.S3, "S2"}, cid
        assert debug in (None, "train_serial"), cid
    # both variants of every training step that forks a library stream
    forked = {c[0][:-len("-fork")] for c in G.CASES if c[0].endswith("-fork")}
    assert forked and forked == {c[0][:-len("-serial")] for c in G.CASES if c[0].endswith("-serial")}
    # every training step is captured in both variants
    assert all(G.S3 in c[3] for c in G.CASES if c[4] or c[0].endswith("-fork") if "marked" not in c[0])
    # the marked backward is never captured: its events are for the host and other streams
    assert all(G.S3 not in c[3] for c in G.CASES if "kdlae_tt_backward_marked" in c[1])
