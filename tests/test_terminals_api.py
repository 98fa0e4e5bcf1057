"""ABI 6: dsl_settings.max_terminals, dsl_result.terminals and dsl_terminal -- the header, the ctypes
mirrors and SearchSettings.maxTerminals (no device needed)."""
import ctypes
import os
import re
import subprocess

from dslabs_amd import SearchSettings, _lib
from dslabs_amd.protocols import PingPong

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dslabs_hip.h")).read()


def _struct_body(name):
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} %s;" % name, HEADER, re.S)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_terminal_list():
    assert re.search(r"#define DSL_ABI_VERSION 6\b", HEADER)
    settings = _struct_body("dsl_settings")
    # appended after the last ABI 5 field, so every earlier offset stays
    assert re.search(r"int32_t check_sample;\s*int32_t max_terminals;\s*int32_t reserved;\s*$", settings)
    result = _struct_body("dsl_result")
    assert re.search(r"dsl_event first_not_idempotent;\s*uint64_t terminals_total;\s*int32_t n_terminals;\s*"
                     r"int32_t \w+;\s*dsl_terminal\* terminals;\s*$", result)
    terminal = _struct_body("dsl_terminal")
    assert re.search(r"int32_t end_condition;\s*int32_t predicate_index;\s*int32_t trace_len;\s*int32_t reserved;\s*"
                     r"dsl_event\* trace;\s*uint8_t\* state;\s*$", terminal)
    # no new entry point: the list comes back in dsl_result and dsl_result_free releases it
    assert len(re.findall(r"^(?:int|void|const char\*) (dsl_\w+)\(", HEADER, re.M)) == len(_lib.EXPORTED)


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    """sizeof / offsetof of the structs ABI 6 changed, compiled from the header with gcc."""
    structs = {"dsl_settings": ["do_checks", "check_sample", "max_terminals", "reserved"],
               "dsl_result": ["first_not_idempotent", "terminals_total", "n_terminals", "terminals"],
               "dsl_terminal": ["end_condition", "predicate_index", "trace_len", "reserved", "trace", "state"]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dslabs_hip.h"', "int main(void) {"]
    for st, fields in structs.items():
        src.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f in fields:
            src.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "abi6.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi6"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    for st, fields in structs.items():
        cls = getattr(_lib, st)
        assert ctypes.sizeof(cls) == int(got[st]), st
        for f in fields:
            assert getattr(cls, f).offset == int(got[f"{st}.{f}"]), (st, f)
    # the new settings fields are the struct's tail
    assert _lib.dsl_settings.max_terminals.offset == _lib.dsl_settings.check_sample.offset + 4
    assert ctypes.sizeof(_lib.dsl_settings) == _lib.dsl_settings.reserved.offset + 4


def test_binding_and_library_agree_on_abi_6():
    assert _lib.DSL_ABI_VERSION == 6
    assert _lib.load().dsl_abi_version() == 6


def test_max_terminals_is_encoded_and_part_of_the_signature():
    state = PingPong(1, 2).initial_state()
    s = SearchSettings()
    assert s._encode(state).max_terminals == 0  # off: the reported terminal only
    sig0, enc0 = s._signature(state), s._encode(state)
    assert s.maxTerminals(7) is s
    assert s._signature(state) != sig0
    enc1 = s._encode(state)
    assert enc1 is not enc0 and enc1.max_terminals == 7 and enc1.reserved == 0  # no stale encoding reused
    assert s._encode(state) is enc1
    assert s.clone()._encode(state).max_terminals == 7
    assert s.maxTerminals(0)._encode(state).max_terminals == 0


def test_results_without_a_list():
    from dslabs_amd.search import EndCondition, SearchResults
    r = SearchResults(EndCondition.SPACE_EXHAUSTED, 1, [1], 0, 0, None, None, 0.0, 0)
    assert r.terminals() == [] and r.numTerminals() == 0
    assert r.invariantViolatingStates() == [] and r.goalMatchingStates() == [] and r.exceptionalStates() == []
