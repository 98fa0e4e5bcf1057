"""Host-side mirror of the reference's search API, running the MI355X engine.

Mirrors (names, argument meaning, error behaviour) of, relative to
/root/reference/framework/tst/dslabs/framework/testing:
  * search/Search.java:390-395            ``Search.bfs(initialState, settings)``
  * search/SearchSettings.java:43-199     ``SearchSettings`` (maxDepth, addGoal/addPrune, ...)
  * TestSettings.java:46-245              invariants, maxTimeSecs, link/sender/receiver filters,
                                          partition, deliverTimers
  * search/SearchResults.java:34-88       ``SearchResults`` / ``EndCondition``
  * StatePredicate.java:52-83, :382-396   standard predicates and ``negate()``

Every search runs on the GPU through libdslabs_hip.so; there is no CPU fallback.
Method names keep the reference's camelCase so that tests read like the reference's tests.
"""
from __future__ import annotations

import ctypes
import enum
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

from . import _lib
from ._lib import check


class EndCondition(enum.IntEnum):
    EXCEPTION_THROWN = 0
    INVARIANT_VIOLATED = 1
    GOAL_FOUND = 2
    SPACE_EXHAUSTED = 3
    TIME_EXHAUSTED = 4


# dsl_predicate_id
PRED_RESULTS_OK = 1
PRED_CLIENTS_DONE = 2
PRED_CLIENT_DONE = 3
PRED_NONE_DECIDED = 4
PRED_CLIENT_HAS_RESULTS = 5


# combinators (dsl_predicate_id DSL_PRED_AND / _OR / _IMPLIES)
PRED_AND = 900
PRED_OR = 901
PRED_IMPLIES = 902


# the generic field leaf (DSL_PRED_FIELD) and its comparisons (DSL_CMP_*, include/dslabs_hip.h)
PRED_FIELD = 950
CMP_EQ, CMP_NE, CMP_LT, CMP_GE, CMP_LE, CMP_GT = 0, 1, 2, 3, 4, 5
_CMP_TEXT = {CMP_EQ: "==", CMP_NE: "!=", CMP_LT: "<", CMP_GE: ">=", CMP_LE: "<=", CMP_GT: ">"}


def field_desc(node: int, bit: int, width: int) -> int:
    """DSL_FIELD_DESC: bit (bits 0-15) | width << 16 (bits 16-21) | node << 22 (bits 22-26)."""
    return (node << 22) | (width << 16) | bit


def field_desc_decode(desc: int) -> tuple:
    """(node, bit, width) of a descriptor (DSL_FIELD_NODE / _BIT / _WIDTH)."""
    return (desc >> 22) & 0x1F, desc & 0xFFFF, (desc >> 16) & 0x3F


def field_arg0(desc: int, cmp: int, rhs_is_field: bool) -> int:
    """DSL_FIELD_ARG0: descriptor | comparison << 32 | (right operand is a field) << 35."""
    return desc | (cmp << 32) | ((1 if rhs_is_field else 0) << 35)


def field_arg0_decode(arg0: int) -> tuple:
    """(descriptor, comparison, rhs_is_field) of a field leaf's arg0."""
    return arg0 & 0xFFFFFFFF, (arg0 >> 32) & 7, bool((arg0 >> 35) & 1)


# the generic network leaf (DSL_PRED_NET) and its conditions (DSL_PRED_REC_COND)
PRED_NET = 951
PRED_REC_COND = 952
MAX_NET_CONDS = 8         # DSL_MAX_NET_CONDS: conditions of one leaf
MAX_NET_CONDS_TOTAL = 32  # DSL_MAX_NET_CONDS_TOTAL: conditions of all the leaves of one search


def rec_arg0(bit: int, width: int, cmp: int) -> int:
    """DSL_REC_ARG0: bit (bits 0-15) | width << 16 (bits 16-21) | comparison << 32 (bits 32-34)."""
    return bit | (width << 16) | (cmp << 32)


def rec_arg0_decode(arg0: int) -> tuple:
    """(bit, width, comparison) of a record condition's arg0 (DSL_REC_ARG0_BIT / _WIDTH / _CMP)."""
    return arg0 & 0xFFFF, (arg0 >> 16) & 0x3F, (arg0 >> 32) & 7


# The step leaves (DSL_PRED_STEP_*, include/dslabs_hip.h): legal only in a step invariant
PRED_STEP_FIELD = 953
PRED_STEP_SENT = 954
PRED_STEP_EVENT = 955
STEP_LHS_NEW_BIT, STEP_RHS_NEW_BIT = 36, 37
_STEP_LEAVES = (PRED_STEP_FIELD, PRED_STEP_SENT, PRED_STEP_EVENT)


def step_field_arg0(desc: int, cmp: int, rhs_is_field: bool, lhs_new: bool, rhs_new: bool) -> int:
    """DSL_STEP_FIELD_ARG0"""
    return field_arg0(desc, cmp, rhs_is_field) | (1 << STEP_LHS_NEW_BIT if lhs_new else 0) | \
        (1 << STEP_RHS_NEW_BIT if rhs_new else 0)


def step_field_arg0_decode(arg0: int) -> tuple:
    """(descriptor, comparison, rhs_is_field, lhs_new, rhs_new): DSL_FIELD_ARG0_* / DSL_STEP_ARG0_*"""
    return field_arg0_decode(arg0 & ((1 << 36) - 1)) + (bool((arg0 >> STEP_LHS_NEW_BIT) & 1),
                                                       bool((arg0 >> STEP_RHS_NEW_BIT) & 1))


class StatePredicate:
    """A named state predicate evaluated on the device (StatePredicate.java).

    ``address_args`` names the positional args that are node addresses; they are resolved
    to node indices against the search state's address table when the search starts.
    Combinators follow StatePredicate.and / or / implies (StatePredicate.java:397-431); ``and``
    and ``or`` are Python keywords, so they are spelled ``and_`` / ``or_`` here.
    """

    def __init__(self, name: str, pred_id: int, arg0=0, arg1=0, negated: bool = False,
                 address_args: Sequence[int] = (), operands: Sequence["StatePredicate"] = (),
                 conds: Sequence["RecCond"] = ()):
        self.name = name
        self.conds = tuple(conds)  # PRED_NET: the record conditions (pool entries when encoded)
        self.pred_id = pred_id
        self.arg0 = arg0
        self.arg1 = arg1
        self.negated = negated
        self.address_args = tuple(address_args)
        self.operands = tuple(operands)

    def negate(self) -> "StatePredicate":
        # StatePredicate.negate(): "¬(name)" or strip an existing "¬(...)".
        if self.name.startswith("¬(") and self.name.endswith(")"):
            name = self.name[2:-1]
        else:
            name = f"¬({self.name})"
        return StatePredicate(name, self.pred_id, self.arg0, self.arg1, not self.negated, self.address_args,
                              self.operands, self.conds)

    def and_(self, other: "StatePredicate") -> "StatePredicate":
        return StatePredicate(f"({self.name}) ∧ ({other.name})", PRED_AND, operands=(self, other))

    def or_(self, other: "StatePredicate") -> "StatePredicate":
        return StatePredicate(f"({self.name}) ∨ ({other.name})", PRED_OR, operands=(self, other))

    def implies(self, other: "StatePredicate") -> "StatePredicate":
        return StatePredicate(f"({self.name}) → ({other.name})", PRED_IMPLIES, operands=(self, other))

    def _encode(self, state: "SearchState", pool: list) -> _lib.dsl_predicate:
        """The C ABI form; a combinator's operands and a network leaf's conditions are appended to
        ``pool`` (dsl_settings.pool)."""
        if self.pred_id in (PRED_NET, PRED_STEP_SENT):
            first = len(pool)
            for c in self.conds:  # consecutive pool entries
                pool.append(_lib.dsl_predicate(PRED_REC_COND, 0, rec_arg0(c.bit, c.width, c.cmp), c.const))
            return _lib.dsl_predicate(self.pred_id, 1 if self.negated else 0, first, len(self.conds))
        if self.operands:
            idx = []
            for op in self.operands:
                pool.append(op._encode(state, pool))
                idx.append(len(pool) - 1)
            return _lib.dsl_predicate(self.pred_id, 1 if self.negated else 0, idx[0], idx[1])
        args = [self.arg0, self.arg1]
        for i in self.address_args:
            args[i] = state.protocol.address_index(args[i])
        return _lib.dsl_predicate(self.pred_id, 1 if self.negated else 0, int(args[0]), int(args[1]))

    def __repr__(self) -> str:
        return self.name


RESULTS_OK = StatePredicate("Clients got expected results", PRED_RESULTS_OK)
CLIENTS_DONE = StatePredicate("All clients' workloads finished", PRED_CLIENTS_DONE)
NONE_DECIDED = StatePredicate("No results returned", PRED_NONE_DECIDED)


def clientDone(address: str) -> StatePredicate:
    return StatePredicate(f"{address}'s workload finished", PRED_CLIENT_DONE, address, address_args=(0,))


def clientHasResults(address: str, numResults: int) -> StatePredicate:
    return StatePredicate(f"{address} received {numResults} results", PRED_CLIENT_HAS_RESULTS, address,
                          numResults, address_args=(0,))


class FieldRef:
    """``width`` bits from bit ``bit`` of one node's packed words: a named field of a protocol's
    node (``IRProtocol.field`` / ``length``), a part of one (``bits``), or a raw bit range
    (``Protocol.raw_field``). Comparing it with an int or with another FieldRef (``eq / ne / lt /
    le / gt / ge`` or the operators; unsigned) gives a StatePredicate the engine judges on the
    device: the user-written predicate of StatePredicate.statePredicate (StatePredicate.java:168-176)."""

    def __init__(self, protocol, node: int, bit: int, width: int, name: str):
        self.protocol, self.node, self.bit, self.width, self.name = protocol, node, bit, width, name

    def desc(self) -> int:
        return field_desc(self.node, self.bit, self.width)

    def bits(self, lo: int, width: int) -> "FieldRef":
        """The sub-field of ``width`` bits from bit ``lo`` of this field."""
        if lo < 0 or width < 1 or lo + width > self.width:
            raise ValueError(f"bits({lo}, {width}) outside {self.name} ({self.width} bits)")
        return FieldRef(self.protocol, self.node, self.bit + lo, width, f"{self.name}[{lo}:{lo + width}]")

    def _cmp(self, cmp: int, other) -> StatePredicate:
        if isinstance(other, StepFieldRef):
            raise TypeError(f"{self.name}: in a step predicate both sides name their state: wrap this field in "
                            f"old(...) or new(...) to compare it with {other.name}")
        if isinstance(other, FieldRef):
            if other.protocol is not self.protocol:
                raise ValueError(f"{self.name} and {other.name} belong to different protocol objects")
            return StatePredicate(f"{self.name} {_CMP_TEXT[cmp]} {other.name}", PRED_FIELD,
                                  field_arg0(self.desc(), cmp, True), other.desc())
        if isinstance(other, bool) or not isinstance(other, int):
            raise TypeError(f"{self.name}: compare with an int or a FieldRef, not {type(other).__name__}")
        if other < 0 or other >= 1 << 32:
            raise ValueError(f"{self.name}: constant {other} does not fit in 32 unsigned bits")
        return StatePredicate(f"{self.name} {_CMP_TEXT[cmp]} {other}", PRED_FIELD,
                              field_arg0(self.desc(), cmp, False), other)

    def eq(self, other) -> StatePredicate:
        return self._cmp(CMP_EQ, other)

    def ne(self, other) -> StatePredicate:
        return self._cmp(CMP_NE, other)

    def lt(self, other) -> StatePredicate:
        return self._cmp(CMP_LT, other)

    def le(self, other) -> StatePredicate:
        return self._cmp(CMP_LE, other)

    def gt(self, other) -> StatePredicate:
        return self._cmp(CMP_GT, other)

    def ge(self, other) -> StatePredicate:
        return self._cmp(CMP_GE, other)

    __eq__, __ne__, __lt__, __le__, __gt__, __ge__ = eq, ne, lt, le, gt, ge
    __hash__ = object.__hash__

    def __repr__(self) -> str:
        return self.name


class StepFieldRef:
    """``old(ref)`` / ``new(ref)``: a FieldRef read from the parent or from the successor of a step.
    Comparing it with an int, ``old(..)`` or ``new(..)`` gives a step leaf (DSL_PRED_STEP_FIELD) for
    ``SearchSettings.addStepInvariant``; a bare FieldRef on the other side is an error."""

    def __init__(self, ref: FieldRef, is_new: bool):
        if not isinstance(ref, FieldRef):
            raise TypeError(f"{'new' if is_new else 'old'}(...) wraps a FieldRef, not {type(ref).__name__}")
        self.ref, self.is_new = ref, bool(is_new)
        self.name = f"{'new' if is_new else 'old'}({ref.name})"

    def bits(self, lo: int, width: int) -> "StepFieldRef":
        return StepFieldRef(self.ref.bits(lo, width), self.is_new)

    def _cmp(self, cmp: int, other) -> "StatePredicate":
        if isinstance(other, StepFieldRef):
            if other.ref.protocol is not self.ref.protocol:
                raise ValueError(f"{self.name} and {other.name} belong to different protocol objects")
            return StatePredicate(f"{self.name} {_CMP_TEXT[cmp]} {other.name}", PRED_STEP_FIELD,
                                  step_field_arg0(self.ref.desc(), cmp, True, self.is_new, other.is_new), other.ref.desc())
        if isinstance(other, FieldRef):
            raise TypeError(f"{self.name}: in a step predicate both sides name their state: wrap {other.name} in "
                            "old(...) or new(...)")
        if isinstance(other, bool) or not isinstance(other, int):
            raise TypeError(f"{self.name}: compare with an int, old(...) or new(...), not {type(other).__name__}")
        if other < 0 or other >= 1 << 32:
            raise ValueError(f"{self.name}: constant {other} does not fit in 32 unsigned bits")
        return StatePredicate(f"{self.name} {_CMP_TEXT[cmp]} {other}", PRED_STEP_FIELD,
                              step_field_arg0(self.ref.desc(), cmp, False, self.is_new, False), other)

    def eq(self, other):
        return self._cmp(CMP_EQ, other)

    def ne(self, other):
        return self._cmp(CMP_NE, other)

    def lt(self, other):
        return self._cmp(CMP_LT, other)

    def le(self, other):
        return self._cmp(CMP_LE, other)

    def gt(self, other):
        return self._cmp(CMP_GT, other)

    def ge(self, other):
        return self._cmp(CMP_GE, other)

    __eq__, __ne__, __lt__, __le__, __gt__, __ge__ = eq, ne, lt, le, gt, ge
    __hash__ = object.__hash__

    def __repr__(self) -> str:
        return self.name


def old(ref: FieldRef) -> StepFieldRef:
    """``ref`` as the step's parent state holds it."""
    return StepFieldRef(ref, False)


def new(ref: FieldRef) -> StepFieldRef:
    """``ref`` as the step's successor holds it."""
    return StepFieldRef(ref, True)


def make_field_ref(protocol, address, bit: int, width: int, name: str) -> FieldRef:
    """A checked FieldRef: a known address, 1..32 bits inside one 32-bit word and (where the
    protocol's words per node are known: ``protocol.node_words``) inside the node."""
    node = protocol.address_index(address)
    if not 0 <= node < len(protocol.addresses):
        raise ValueError(f"unknown address {address!r}")
    if not 1 <= width <= 32:
        raise ValueError(f"{name}: width {width} outside 1..32")
    if bit < 0 or bit >= 1 << 16:
        raise ValueError(f"{name}: bit {bit} outside the node")
    if (bit & 31) + width > 32:
        raise ValueError(f"{name}: bits {bit}..{bit + width - 1} straddle a 32-bit word")
    nw = getattr(protocol, "node_words", 0)
    if nw and bit + width > 32 * nw:
        raise ValueError(f"{name}: bits {bit}..{bit + width - 1} beyond the node's {32 * nw} bits")
    return FieldRef(protocol, node, bit, width, name)


class RecCond:
    """One condition of a message pattern: ``width`` bits from bit ``bit`` of the packed record
    compared (unsigned, DSL_CMP_*) with a constant."""

    def __init__(self, bit: int, width: int, cmp: int, const: int, text: str):
        self.bit, self.width, self.cmp, self.const, self.text = bit, width, cmp, const, text

    def holds(self, rec: int) -> bool:
        x = (rec >> self.bit) & ((1 << self.width) - 1)
        return {CMP_EQ: x == self.const, CMP_NE: x != self.const, CMP_LT: x < self.const, CMP_GE: x >= self.const,
                CMP_LE: x <= self.const, CMP_GT: x > self.const}[self.cmp]

    def __repr__(self) -> str:
        return self.text


class RecFieldRef:
    """A bit field of a message's packed record (``MessagePattern.field`` / ``raw_field``):
    comparing it with an int gives a RecCond for ``MessagePattern.where``."""

    def __init__(self, bit: int, width: int, name: str):
        self.bit, self.width, self.name = bit, width, name

    def _cmp(self, cmp: int, other) -> RecCond:
        if isinstance(other, bool) or not isinstance(other, int):
            raise TypeError(f"{self.name}: compare with an int, not {type(other).__name__}")
        if other < 0 or other >= 1 << self.width:
            raise ValueError(f"{self.name}: constant {other} does not fit in the field's {self.width} bits")
        return RecCond(self.bit, self.width, cmp, other, f"{self.name} {_CMP_TEXT[cmp]} {other}")

    def eq(self, other) -> RecCond:
        return self._cmp(CMP_EQ, other)

    def ne(self, other) -> RecCond:
        return self._cmp(CMP_NE, other)

    def lt(self, other) -> RecCond:
        return self._cmp(CMP_LT, other)

    def le(self, other) -> RecCond:
        return self._cmp(CMP_LE, other)

    def gt(self, other) -> RecCond:
        return self._cmp(CMP_GT, other)

    def ge(self, other) -> RecCond:
        return self._cmp(CMP_GE, other)

    __eq__, __ne__, __lt__, __le__, __gt__, __ge__ = eq, ne, lt, le, gt, ge
    __hash__ = object.__hash__

    def __repr__(self) -> str:
        return self.name


def _check_rec_field(name: str, bit: int, width: int, rec_bits: int) -> None:
    if isinstance(bit, bool) or isinstance(width, bool) or not isinstance(bit, int) or not isinstance(width, int):
        raise TypeError(f"{name}: bit and width are ints")
    if not 1 <= width <= 32:
        raise ValueError(f"{name}: width {width} outside 1..32")
    if bit < 0 or bit + width > rec_bits:
        raise ValueError(f"{name}: bits {bit}..{bit + width - 1} outside the record's {rec_bits} bits")


class MessagePattern:
    """Messages of one type, optionally from / to given addresses (``IRProtocol.message``), or any
    record of a hand-written protocol (``Protocol.raw_message``). ``where(cond, ...)`` gives the
    StatePredicate "the network (dropped messages included) holds a message of this pattern that
    satisfies every condition": StatePredicate.containsMessageMatching (StatePredicate.java:139-149)
    for a conjunction of field comparisons, judged on the device (DSL_PRED_NET)."""

    def __init__(self, protocol, label: str, base: Sequence[RecCond], fields, rec_bits: int):
        self.protocol, self.label, self.base, self.fields, self.rec_bits = protocol, label, tuple(base), fields, rec_bits

    def field(self, name: str) -> RecFieldRef:
        """Field ``name`` of the message type (fields pack from bit 0 in declaration order)."""
        if self.fields is None:
            raise ValueError(f"{self.label}: a raw message has no named fields (use raw_field)")
        if name not in self.fields:
            raise ValueError(f"{self.label} has no field {name!r}")
        bit, width = self.fields[name]
        _check_rec_field(f"{self.label}.{name}", bit, width, self.rec_bits)
        return RecFieldRef(bit, width, name)

    def raw_field(self, bit: int, width: int) -> RecFieldRef:
        """``width`` bits (1..32) from bit ``bit`` of the packed record, for a caller who knows
        the layout (csrc/protocols/*.hpp)."""
        _check_rec_field(f"{self.label}.bits[{bit}:{bit + width}]", bit, width, self.rec_bits)
        return RecFieldRef(bit, width, f"bits[{bit}:{bit + width}]")

    def sent(self, *conds: RecCond) -> StatePredicate:
        """A step leaf (SearchSettings.addStepInvariant): the step ADDED to the network a message of
        this pattern satisfying every condition (DSL_PRED_STEP_SENT). The network is a set: a
        message the parent already holds is not added by sending it again."""
        p = self.where(*conds)
        return StatePredicate("sent" + p.name[len("contains"):], PRED_STEP_SENT, conds=p.conds)

    def where(self, *conds: RecCond) -> StatePredicate:
        for c in conds:
            if not isinstance(c, RecCond):
                raise TypeError(f"{self.label}.where: a condition is a comparison of a field of the message "
                                f"with an int, not {type(c).__name__}")
            if c.bit + c.width > self.rec_bits:
                raise ValueError(f"{self.label}.where: {c.text} lies outside the record's {self.rec_bits} bits")
        allc = self.base + tuple(conds)
        if not allc:
            raise ValueError(f"{self.label}.where: no condition at all")
        if len(allc) > MAX_NET_CONDS:
            raise ValueError(f"{self.label}.where: {len(allc)} conditions, at most {MAX_NET_CONDS} "
                             "(message type and addresses included)")
        name = f"contains {self.label}" + (f"({', '.join(c.text for c in conds)})" if conds else "")
        return StatePredicate(name, PRED_NET, conds=allc)

    def __repr__(self) -> str:
        return self.label


def message_matches(state: "SearchState", pred: StatePredicate) -> List[int]:
    """The records of ``state``'s network(), dropped ones included, that satisfy every condition of
    the message predicate ``pred`` (negation ignored), decoded on the host: empty when the
    device's leaf is false."""
    if pred.pred_id != PRED_NET:
        raise ValueError(f"{pred.name!r} is not a message predicate")
    return [r for r in state.records() if all(c.holds(r) for c in pred.conds)]


def statePredicate(name: str, pred: StatePredicate) -> StatePredicate:
    """StatePredicate.statePredicate(name, fn) (StatePredicate.java:168-176) for a predicate built
    from field comparisons and combinators: the same predicate under ``name``."""
    return StatePredicate(name, pred.pred_id, pred.arg0, pred.arg1, pred.negated, pred.address_args, pred.operands,
                          pred.conds)


def _fold(preds, op: str, what: str) -> StatePredicate:
    preds = list(preds)
    if not preds:
        raise ValueError(f"{what} of no predicates")
    out = preds[0]
    for p in preds[1:]:
        out = getattr(out, op)(p)
    return out


def allOf(preds) -> StatePredicate:
    """The conjunction of a non-empty list, folded left with ``and_``."""
    return _fold(preds, "and_", "allOf")


def anyOf(preds) -> StatePredicate:
    """The disjunction of a non-empty list, folded left with ``or_``."""
    return _fold(preds, "or_", "anyOf")


def field_value(state: "SearchState", ref: FieldRef) -> int:
    """The value of ``ref`` in a state's packed bytes (node i is words [i * node_words,
    (i + 1) * node_words) of the row, little-endian 32-bit words): what the device's field leaf
    reads, decoded on the host."""
    nw = getattr(state.protocol, "node_words", 0)
    if not nw:
        raise ValueError(f"{type(state.protocol).__name__} does not declare node_words")
    packed = state._packed_now()
    w = (ref.node * nw + (ref.bit >> 5)) * 4
    word = int.from_bytes(packed[w:w + 4], "little")
    return (word >> (ref.bit & 31)) & ((1 << ref.width) - 1)


@dataclass
class PredicateResult:
    """StatePredicate.PredicateResult: which predicate fired and its value."""
    predicate: StatePredicate
    value: Optional[bool]

    def errorMessage(self) -> str:
        verb = "matches" if self.value else "violates"
        return f'State {verb} "{self.predicate.name}"'


_NO_WATCHES = (b"", None, 0, None, 0)  # SearchSettings._encode_watches of a search without watches


def _step_leaf_in(p: StatePredicate) -> Optional[StatePredicate]:
    """The first step leaf of a predicate tree, or None."""
    if p.pred_id in _STEP_LEAVES:
        return p
    for o in p.operands:
        f = _step_leaf_in(o)
        if f is not None:
            return f
    return None


def _no_step_leaf(p: StatePredicate, what: str) -> None:
    f = _step_leaf_in(p)
    if f is not None:
        raise ValueError(f"{what}: {f.name!r} is a step leaf: it is legal only in a step invariant (addStepInvariant)")


def _has_pred(p: StatePredicate, pred_id: int) -> bool:
    return p.pred_id == pred_id or any(_has_pred(o, pred_id) for o in p.operands)


@dataclass
class StepViolation:
    """SearchResults.stepViolation(): the reported violating edge of a search with step invariants."""
    index: int                 # the lowest violated step invariant of the edge
    name: str
    depth: int                 # depth(parent) + 1
    parent: "SearchState"
    state: "SearchState"
    event: str                 # the edge's event, decoded
    edges: int                 # the level's violating edges
    perInvariant: List[int]    # ... per step invariant (an edge counts for every one it violates)


class SearchSettings:
    """SearchSettings + TestSettings (fluent setters return self)."""

    def __init__(self):
        self._invariants: List[StatePredicate] = []
        self._goals: List[StatePredicate] = []
        self._prunes: List[StatePredicate] = []
        self._max_depth = -1
        self._max_time_secs = -1
        self._network_active = True
        self._link = {}
        self._sender = {}
        self._receiver = {}
        self._deliver_timers = True
        self._timers_active = {}
        # engine capacity knobs (dsl_settings): the visited table's first size (2^k slots; 0 = 2^20,
        # it grows), a cap on a level's frontier (0 = none), and the device memory the visited
        # table may grow to (bytes; 0 = no limit)
        self.table_log2_slots = 0
        self.max_frontier_states = 0
        self.memory_budget_bytes = 0
        # GlobalSettings.doErrorChecks / doAllChecks (Search.java:201-220): a sample of every level's
        # new states re-derived on the host (determinism) and, for doAllChecks, message deliveries
        # stepped twice (idempotence); counts in SearchResults.checks
        self.do_checks = _lib.DSL_CHECKS_NONE
        self.check_sample = 0
        # dsl_settings.max_terminals: every terminal state of the level that ends a BFS, at most
        # this many listed (SearchResults.terminals()); 0 = only the reported one
        self.max_terminals = 0
        # watches (dsl_set_watches): predicates that are only counted, per depth, over every state
        # the search discovers (SearchResults.watchCounts()); they change nothing else
        self._watches: List[StatePredicate] = []
        # per watch: the search also returns a witness state of its first hit (dsl_set_watch_witnesses)
        self._witness: List[bool] = []
        # the event census (dsl_set_event_census): per level, the events applied per handler class
        # and destination node (SearchResults.eventCensus()); it changes nothing else
        self._event_census = False
        # step invariants (dsl_set_step_invariants): predicates over an edge (parent, event, successor)
        self._step_invariants: List[StatePredicate] = []

    def addStepInvariant(self, p: StatePredicate) -> "SearchSettings":
        """A predicate every step (parent, event, successor) of the search must satisfy, built from
        ``old(ref) / new(ref)`` comparisons, ``MessagePattern.sent``, ``Protocol.delivered``, field
        comparisons and named predicates (both on the successor) and the combinators; at most 8. A
        step that changes nothing is exempt. The search ends INVARIANT_VIOLATED at the first level
        with a violated step (SearchResults.stepViolation). BFS on one shard."""
        if len(self._step_invariants) >= _lib.DSL_MAX_STEP_INVARIANTS:
            raise ValueError(f"too many step invariants: at most {_lib.DSL_MAX_STEP_INVARIANTS} in one search")
        if _has_pred(p, PRED_NET):
            raise ValueError(f"addStepInvariant: {p.name!r} holds a message predicate over the whole network "
                             "(MessagePattern.where), which a step invariant does not support: use .sent(...)")
        self._step_invariants.append(p)
        return self

    def clearStepInvariants(self) -> "SearchSettings":
        self._step_invariants.clear()
        return self

    def stepInvariants(self) -> List[StatePredicate]:
        return list(self._step_invariants)

    def _encode_steps(self, state: "SearchState") -> tuple:
        """``(key, preds, n, pool, n_pool)`` as dsl_set_step_invariants takes them (see _encode_watches)."""
        if not self._step_invariants:
            return _NO_WATCHES
        sig = (state.protocol, tuple(self._step_invariants))
        cached = self.__dict__.get("_step_cache")
        if cached is not None and cached[0] == sig:
            return cached[1]
        pool: list = []
        preds = [p._encode(state, pool) for p in self._step_invariants]
        if len(pool) > _lib.DSL_MAX_POOL:
            raise ValueError(f"too many combinator operands and message conditions in the step invariants: {len(pool)} "
                             f"pool entries, at most {_lib.DSL_MAX_POOL}")
        w = (_lib.dsl_predicate * _lib.DSL_MAX_STEP_INVARIANTS)(*preds)
        pl = (_lib.dsl_predicate * _lib.DSL_MAX_POOL)(*pool)
        enc = (bytes(w) + bytes(pl), w, len(preds), pl, len(pool))
        self.__dict__["_step_cache"] = (sig, enc)
        return enc

    def eventCensus(self, on: bool = True) -> "SearchSettings":
        """Counts, per expanded level, the events applied per (handler class, destination node):
        how many were delivered, led back to their parent, threw, and reached a state not
        discovered before that level (SearchResults.eventCensus / eventTotals / eventRows). The
        search itself is unchanged. BFS on one shard."""
        self._event_census = bool(on)
        return self

    def addWatch(self, p: StatePredicate, witness: bool = False) -> "SearchSettings":
        """Counts, per depth, the newly discovered states in which ``p`` holds, without ending or
        cutting the search (an invariant, goal or prune does one or the other). Any predicate the
        engine accepts; at most 8 per search. BFS on one shard. ``witness=True`` also asks for one
        state of the first depth at which ``p`` held, with a shortest trace
        (SearchResults.watchWitness): what a goal search's goalMatchingState() gives."""
        if len(self._watches) >= _lib.DSL_MAX_WATCHES:
            raise ValueError(f"too many watches: at most {_lib.DSL_MAX_WATCHES} in one search")
        _no_step_leaf(p, "addWatch")
        self._watches.append(p)
        self._witness.append(bool(witness))
        return self

    def clearWatches(self) -> "SearchSettings":
        self._watches.clear()
        self._witness.clear()
        return self

    def _witness_mask(self) -> int:
        """dsl_set_watch_witnesses' mask: bit w = watch w wants a witness."""
        return sum(1 << w for w, f in enumerate(self._witness) if f)

    def watches(self) -> List[StatePredicate]:
        return list(self._watches)

    def _encode_watches(self, state: "SearchState") -> tuple:
        """The C ABI form of the watches, ``(key, watches, n, pool, n_pool)``: two dsl_predicate
        arrays as dsl_set_watches takes them and a key equal exactly when they are (the engine is
        told only when it differs from what it holds); the same tuple again while the watches did
        not change."""
        if not self._watches:
            return _NO_WATCHES
        sig = (state.protocol, tuple(self._watches))
        cached = self.__dict__.get("_watch_cache")
        if cached is not None and cached[0] == sig:
            return cached[1]
        pool: list = []
        preds = [p._encode(state, pool) for p in self._watches]
        if len(pool) > _lib.DSL_MAX_POOL:
            raise ValueError(f"too many combinator operands and message conditions in the watches: {len(pool)} "
                             f"pool entries, at most {_lib.DSL_MAX_POOL}")
        w = (_lib.dsl_predicate * _lib.DSL_MAX_WATCHES)(*preds)
        pl = (_lib.dsl_predicate * _lib.DSL_MAX_POOL)(*pool)
        enc = (bytes(w) + bytes(pl), w, len(preds), pl, len(pool))
        self.__dict__["_watch_cache"] = (sig, enc)
        return enc

    def maxTerminals(self, n: int) -> "SearchSettings":
        """List every terminal state of the level that ends a BFS (all shortest counterexamples,
        all goal states of a staged search), at most ``n`` of them; 0 turns the list off."""
        if n < 0:
            raise ValueError("maxTerminals: n must be >= 0")
        self.max_terminals = int(n)
        return self

    def doErrorChecks(self, on: bool = True) -> "SearchSettings":
        self.do_checks = _lib.DSL_CHECKS_ERRORS if on else _lib.DSL_CHECKS_NONE
        return self

    def doAllChecks(self, on: bool = True) -> "SearchSettings":
        self.do_checks = _lib.DSL_CHECKS_ALL if on else _lib.DSL_CHECKS_NONE
        return self

    # TestSettings -------------------------------------------------------------------------
    def addInvariant(self, p: StatePredicate) -> "SearchSettings":
        _no_step_leaf(p, "addInvariant")
        self._invariants.append(p)
        return self

    def clearInvariants(self) -> "SearchSettings":
        self._invariants.clear()
        return self

    def invariants(self) -> List[StatePredicate]:
        return list(self._invariants)

    def maxTimeSecs(self, secs: int) -> "SearchSettings":
        self._max_time_secs = secs
        return self

    def timeLimited(self) -> bool:
        return self._max_time_secs > 0

    def linkActive(self, frm: str, to: str, active: bool) -> "SearchSettings":
        self._link[(frm, to)] = active
        return self

    def senderActive(self, frm: str, active: bool) -> "SearchSettings":
        self._sender[frm] = active
        return self

    def receiverActive(self, to: str, active: bool) -> "SearchSettings":
        self._receiver[to] = active
        return self

    def nodeActive(self, node: str, active: bool) -> "SearchSettings":
        self.receiverActive(node, active)
        return self.senderActive(node, active)

    def networkActive(self, active: bool) -> "SearchSettings":
        self._network_active = active
        return self

    def partition(self, *groups) -> "SearchSettings":
        """TestSettings.partition: network off, links inside each group on.
        Accepts addresses (one group) or sequences of addresses (several groups)."""
        if groups and isinstance(groups[0], str):
            groups = (groups,)
        self._network_active = False
        for g in groups:
            for a in g:
                for b in g:
                    if a != b:
                        self._link[(a, b)] = True
        return self

    def reconnect(self) -> "SearchSettings":
        self._network_active = True
        self._link.clear()
        self._sender.clear()
        self._receiver.clear()
        return self

    def deliverTimers(self, *args) -> "SearchSettings":
        if len(args) == 1:
            self._deliver_timers = bool(args[0])
        else:
            self._timers_active[args[0]] = bool(args[1])
        return self

    def clearDeliverTimers(self) -> "SearchSettings":
        self._deliver_timers = True
        self._timers_active.clear()
        return self

    # SearchSettings ------------------------------------------------------------------------
    def maxDepth(self, depth: int) -> "SearchSettings":
        self._max_depth = depth
        return self

    def depthLimited(self) -> bool:
        return self._max_depth >= 0

    def addGoal(self, p: StatePredicate) -> "SearchSettings":
        _no_step_leaf(p, "addGoal")
        self._goals.append(p)
        return self

    def clearGoals(self) -> "SearchSettings":
        self._goals.clear()
        return self

    def goals(self) -> List[StatePredicate]:
        return list(self._goals)

    def addPrune(self, p: StatePredicate) -> "SearchSettings":
        _no_step_leaf(p, "addPrune")
        self._prunes.append(p)
        return self

    def clearPrunes(self) -> "SearchSettings":
        self._prunes.clear()
        return self

    def prunes(self) -> List[StatePredicate]:
        return list(self._prunes)

    def clone(self) -> "SearchSettings":
        s = SearchSettings()
        s.__dict__.update({k: (v.copy() if isinstance(v, (list, dict)) else v) for k, v in self.__dict__.items()
                           if k not in ("_enc_cache", "_watch_cache", "_step_cache")})
        return s

    # encoding -------------------------------------------------------------------------------
    def _signature(self, state: "SearchState") -> tuple:
        """Everything _encode reads (predicates and protocols by identity: they are immutable)."""
        return (state.protocol, self._max_depth, self._max_time_secs, self._network_active, self._deliver_timers,
                tuple(self._link.items()), tuple(self._sender.items()), tuple(self._receiver.items()),
                tuple(self._timers_active.items()), tuple(self._invariants), tuple(self._goals), tuple(self._prunes),
                self.table_log2_slots, self.max_frontier_states, self.memory_budget_bytes, self.do_checks,
                self.check_sample, self.max_terminals, tuple(self._watches), tuple(self._witness), self._event_census)

    def _encode(self, state: "SearchState") -> _lib.dsl_settings:
        """The C ABI form (dsl_settings); the same object again while nothing it reads changed,
        so a repeated search skips the encoding and the engine skips dsl_set_settings."""
        sig = self._signature(state)
        cached = self.__dict__.get("_enc_cache")
        if cached is not None and cached[0] == sig:
            return cached[1]
        s = self._encode_new(state)
        self.__dict__["_enc_cache"] = (sig, s)
        return s

    def _encode_new(self, state: "SearchState") -> _lib.dsl_settings:
        proto = state.protocol
        s = _lib.dsl_settings()
        s.max_depth = self._max_depth
        s.max_time_ms = max(1, int(round(self._max_time_secs * 1000))) if self._max_time_secs > 0 else -1
        s.network_active = 1 if self._network_active else 0
        s.deliver_timers = 1 if self._deliver_timers else 0
        ctypes.memset(ctypes.addressof(s.link_active), 0xFF, ctypes.sizeof(s.link_active))
        ctypes.memset(ctypes.addressof(s.sender_active), 0xFF, ctypes.sizeof(s.sender_active))
        ctypes.memset(ctypes.addressof(s.receiver_active), 0xFF, ctypes.sizeof(s.receiver_active))
        ctypes.memset(ctypes.addressof(s.timers_active), 0xFF, ctypes.sizeof(s.timers_active))
        for (a, b), v in self._link.items():
            s.link_active[proto.address_index(a)][proto.address_index(b)] = 1 if v else 0
        for a, v in self._sender.items():
            s.sender_active[proto.address_index(a)] = 1 if v else 0
        for a, v in self._receiver.items():
            s.receiver_active[proto.address_index(a)] = 1 if v else 0
        for a, v in self._timers_active.items():
            s.timers_active[proto.address_index(a)] = 1 if v else 0
        pool = []
        for name, lst, arr in (("n_invariants", self._invariants, s.invariants),
                               ("n_goals", self._goals, s.goals), ("n_prunes", self._prunes, s.prunes)):
            if len(lst) > _lib.DSL_MAX_PREDICATES:
                raise ValueError("too many predicates")
            setattr(s, name, len(lst))
            for i, p in enumerate(lst):
                arr[i] = p._encode(state, pool)
        if len(pool) > _lib.DSL_MAX_POOL:
            raise ValueError(f"too many combinator operands and message conditions: {len(pool)} pool entries, "
                             f"at most {_lib.DSL_MAX_POOL}")
        if sum(p.pred_id == PRED_REC_COND for p in pool) > MAX_NET_CONDS_TOTAL:
            raise ValueError(f"too many message conditions in one search: at most {MAX_NET_CONDS_TOTAL}")
        s.n_pool = len(pool)
        for i, p in enumerate(pool):
            s.pool[i] = p
        s.table_log2_slots = self.table_log2_slots
        s.max_frontier_states = self.max_frontier_states
        s.memory_budget_bytes = self.memory_budget_bytes
        s.do_checks = self.do_checks
        s.check_sample = self.check_sample
        s.max_terminals = self.max_terminals
        return s


class SearchState:
    """A search state handle: the protocol configuration plus (optionally) a packed state.

    ``SearchState`` objects for the initial state are made by the protocol builders in
    ``dslabs_amd.protocols``; terminal states come back from a search with their event trace
    (``trace()``), the analogue of the reference's ``previous`` chain.
    """

    DROPPED_CAP = 4096

    def __init__(self, protocol, packed: Optional[bytes] = None, depth: int = 0,
                 events: Optional[List[str]] = None, raw_events=None, dropped=None):
        self.protocol = protocol
        self.packed = packed
        self._depth = depth
        self._events = events or []
        self._raw_events = raw_events or []
        # SearchState.droppedNetwork (SearchState.java:77): records set aside by
        # dropPendingMessages; successors found by a search from this state inherit the set
        self._dropped = list(dropped or [])

    # ---- dropped network (SearchState.java:538-561) ----------------------------------------------
    def _packed_now(self) -> bytes:
        if self.packed is not None:
            return self.packed
        lib = _lib.load()
        desc = self.protocol.desc()
        n = lib.dsl_state_bytes(ctypes.byref(desc))
        check(n if n < 0 else 0, "dsl_state_bytes")
        buf = (ctypes.c_uint8 * n)()
        check(lib.dsl_init_state(ctypes.byref(desc), buf, n), "dsl_init_state")
        return bytes(buf)

    def dropPendingMessages(self) -> None:
        """Every pending message moves to the dropped set: no longer an event, still part of the
        state's message union (SearchState.dropPendingMessages, :538-541). Mutates this state."""
        lib = _lib.load()
        packed = self._packed_now()
        buf = (ctypes.c_uint8 * len(packed)).from_buffer_copy(packed)
        arr = (ctypes.c_uint64 * self.DROPPED_CAP)(*self._dropped)
        n = ctypes.c_int32(len(self._dropped))
        check(lib.dsl_drop_pending_messages(ctypes.byref(self.protocol.desc()), buf, len(packed), arr,
                                            self.DROPPED_CAP, ctypes.byref(n)), "dsl_drop_pending_messages")
        self.packed = bytes(buf)
        self._dropped = list(arr[:n.value])

    def _undrop(self, frm: int, to: int) -> None:
        lib = _lib.load()
        packed = self._packed_now()
        buf = (ctypes.c_uint8 * len(packed)).from_buffer_copy(packed)
        arr = (ctypes.c_uint64 * max(1, len(self._dropped)))(*self._dropped)
        check(lib.dsl_undrop_messages(ctypes.byref(self.protocol.desc()), buf, len(packed), arr,
                                      len(self._dropped), frm, to), "dsl_undrop_messages")
        self.packed = bytes(buf)

    def undropMessages(self) -> None:
        """SearchState.undropMessages (:543-545): every dropped message is pending again."""
        self._undrop(-1, -1)

    def undropMessagesFrom(self, address: str) -> None:
        """SearchState.undropMessagesFrom (:547-553)."""
        self._undrop(self.protocol.address_index(address), -1)

    def undropMessagesTo(self, address: str) -> None:
        """SearchState.undropMessagesTo (:555-561)."""
        self._undrop(-1, self.protocol.address_index(address))

    def droppedMessages(self) -> List[int]:
        """The dropped set as packed records (sorted)."""
        return list(self._dropped)

    def records(self) -> List[int]:
        """network() as packed records (sorted): the state's own and the dropped ones
        (SearchState.java:153-157), what a message predicate reads."""
        c = SearchState(self.protocol, self._packed_now(), dropped=self._dropped)
        c.dropPendingMessages()
        return c.droppedMessages()

    def depth(self) -> int:
        return self._depth

    def trace(self) -> List[str]:
        """Events from the search's initial state to this state (SearchState.trace())."""
        return list(self._events)

    def events(self) -> list:
        """The trace as decoded events (dsl_event copies) from the state the search started at:
        the input of ``Engine.replay`` / ``Search.replay``."""
        return list(self._raw_events)

    def addresses(self) -> List[str]:
        return list(self.protocol.addresses)


class EventCount(NamedTuple):
    """One cell of the event census: the events of one handler class delivered to one node."""
    events: int
    noops: int
    exceptions: int
    fresh: int

    @property
    def revisits(self) -> int:
        """Events that reached a state discovered at the parents' depth or before."""
        return self.events - self.noops - self.exceptions - self.fresh


class SearchResults:
    def __init__(self, end, states, per_depth, initial_depth, max_depth, terminal: Optional[SearchState],
                 predicate: Optional[PredicateResult], elapsed_s: float, successors: int):
        self._end = end
        self.states = states
        self.per_depth = per_depth
        self.initial_depth = initial_depth
        self.max_depth = max_depth
        self._terminal = terminal
        self._predicate = predicate
        self.elapsed_s = elapsed_s
        self.successors = successors
        self.checks = {"run": 0, "not_deterministic": 0, "not_idempotent": 0, "first_not_deterministic": None,
                       "first_not_idempotent": None}
        self._terminals: list = []
        self._terminals_total = 0
        self._watch_counts: List[List[int]] = []
        self._watch_totals: List[int] = []
        self._witnesses: List[Optional[SearchState]] = []
        self._step_edges: List[int] = []
        self._step_violation: Optional[StepViolation] = None
        self._event_rows: list = []       # [level][cls][to] = (events, noops, exceptions, fresh)
        self._event_classes: list = []    # [(name, is_timer)] of the protocol
        self._event_addresses: list = []

    def endCondition(self) -> EndCondition:
        return self._end

    def lastState(self) -> Optional[SearchState]:
        """The state a replay ended in (TraceReplaySearch: also when the trace ran out or an event
        could not be delivered); for a search, its terminal state."""
        return getattr(self, "_last", None) or self._terminal

    def invariantViolatingState(self) -> Optional[SearchState]:
        return self._terminal if self._end == EndCondition.INVARIANT_VIOLATED else None

    def invariantViolated(self) -> Optional[PredicateResult]:
        return self._predicate if self._end == EndCondition.INVARIANT_VIOLATED else None

    def goalMatchingState(self) -> Optional[SearchState]:
        return self._terminal if self._end == EndCondition.GOAL_FOUND else None

    def goalMatched(self) -> Optional[PredicateResult]:
        return self._predicate if self._end == EndCondition.GOAL_FOUND else None

    def exceptionalState(self) -> Optional[SearchState]:
        return self._terminal if self._end == EndCondition.EXCEPTION_THROWN else None

    def exceptionThrown(self) -> bool:
        return self._end == EndCondition.EXCEPTION_THROWN

    # every terminal of the level that ended a BFS (SearchSettings.maxTerminals) ----------------
    def terminals(self) -> list:
        """``(EndCondition, PredicateResult | None, SearchState)`` of every listed terminal state, in
        the engine's order: exceptions, then invariant violations, then goals, each by fingerprint;
        the first entry is the terminal the search reports. Empty unless maxTerminals(n > 0)."""
        return list(self._terminals)

    def numTerminals(self) -> int:
        """All terminal states of that level, also those past the maxTerminals cap."""
        return self._terminals_total

    def _terminals_of(self, end: EndCondition) -> List[SearchState]:
        return [s for e, _, s in self._terminals if e == end]

    def invariantViolatingStates(self) -> List[SearchState]:
        return self._terminals_of(EndCondition.INVARIANT_VIOLATED)

    def goalMatchingStates(self) -> List[SearchState]:
        return self._terminals_of(EndCondition.GOAL_FOUND)

    def exceptionalStates(self) -> List[SearchState]:
        return self._terminals_of(EndCondition.EXCEPTION_THROWN)

    # the watches' census (SearchSettings.addWatch) ----------------------------------------------
    def watchCounts(self) -> List[List[int]]:
        """Per watch, in addWatch order, the newly discovered states in which it held at each depth:
        a list as long as ``per_depth``, index i = depth ``initial_depth + i``. Empty without
        watches, and after a DFS or a replay."""
        return [list(c) for c in self._watch_counts]

    def watchTotal(self, i: int) -> int:
        """All states in which watch ``i`` held, those of a level the time limit cut short included
        (as ``states`` includes them and ``per_depth`` does not)."""
        return self._watch_totals[i]

    def watchFirstDepth(self, i: int) -> Optional[int]:
        """The absolute depth of the first state in which watch ``i`` held; None if none did."""
        for k, c in enumerate(self._watch_counts[i]):
            if c:
                return self.initial_depth + k
        return None

    def watchWitness(self, i: int) -> Optional[SearchState]:
        """The witness of watch ``i`` (``addWatch(p, witness=True)``): the state with the smallest
        fingerprint among those first discovered at ``watchFirstDepth(i)`` in which the watch held,
        with a shortest trace to it -- independent of arrival order, buffer sizes and restarts, and
        usable as the start of the next ``Engine.bfs``. None when none was requested, the watch
        never held in a completed level, or the result is a DFS's or a replay's."""
        n = len(self._watch_counts) if self._watch_counts else _lib.DSL_MAX_WATCHES
        if not 0 <= i < n:
            raise ValueError(f"watchWitness: watch {i} of {n}")
        return self._witnesses[i] if i < len(self._witnesses) else None

    # step invariants (SearchSettings.addStepInvariant) -----------------------------------------
    def stepEdges(self) -> List[int]:
        """Edges judged per completed level (index i: the parents of depth ``initial_depth + i``).
        Empty without step invariants, and after a DFS or a replay."""
        return list(self._step_edges)

    def stepViolation(self) -> Optional[StepViolation]:
        """The reported violating edge, or None. It is there also when an exception or a state
        invariant of the same level outranked it as the search's terminal."""
        return self._step_violation

    # the event census (SearchSettings.eventCensus) ----------------------------------------------
    def eventRows(self) -> list:
        """The raw census: ``rows[i][cls][to] = (events, noops, exceptions, fresh)`` of the events
        applied to the states of depth ``initial_depth + i``, one row per level whose expansion
        completed; ``cls`` indexes ``Protocol.event_classes()``, ``to`` the protocol's addresses.
        Empty without the census, and after a DFS or a replay."""
        return [[[tuple(v) for v in c] for c in row] for row in self._event_rows]

    def eventCensus(self) -> List[dict]:
        """One dict per row, ``{(class_name, address): EventCount}``, of the cells with events."""
        out = []
        for row in self._event_rows:
            d = {}
            for c, cells in enumerate(row):
                for t, v in enumerate(cells):
                    if v[0] > 0:
                        d[(self._event_classes[c][0], self._event_addresses[t])] = EventCount(*v)
            out.append(d)
        return out

    def eventTotals(self) -> dict:
        """``eventCensus()`` summed over the rows."""
        tot: dict = {}
        for d in self.eventCensus():
            for k, v in d.items():
                o = tot.get(k)
                tot[k] = v if o is None else EventCount(*(a + b for a, b in zip(o, v)))
        return tot

    def statesPerSecond(self) -> float:
        return self.states / self.elapsed_s if self.elapsed_s > 0 else float("inf")

    def status(self) -> str:
        # BFS.status() line (Search.java:426-431)
        return "Explored: %d, Depth: %d (%.2fs, %.2fK states/s)" % (
            self.states, self.max_depth, self.elapsed_s, self.statesPerSecond() / 1000.0)


class Engine:
    """One engine (one GPU, or one shard of a multi-GPU search)."""

    def __init__(self, protocol, device: int = -1, rank: int = 0, world_size: int = 1,
                 virtual_shards: int = 0, comm_id: Optional[bytes] = None, host_comm=None,
                 replicate_below: int = -1, rccl_at_world_1: bool = False):
        """rccl_at_world_1: build the RCCL communicator (comm_id) even at world_size 1
        (DSL_CFG_RCCL_AT_WORLD_1), so the collectives run on a one-GPU box."""
        lib = _lib.load()
        self.lib = lib
        self.protocol = protocol
        self.host_comm = host_comm  # keeps the ctypes callbacks alive
        cfg = _lib.dsl_engine_config()
        cfg.device = device
        cfg.rank = rank
        cfg.world_size = world_size
        cfg.virtual_shards = virtual_shards
        cfg.replicate_below = replicate_below
        cfg.flags = _lib.DSL_CFG_RCCL_AT_WORLD_1 if rccl_at_world_1 else 0
        if comm_id is not None:
            ctypes.memmove(cfg.comm_id, comm_id, 128)
        handle = ctypes.c_void_p()
        if host_comm is not None:
            rc = lib.dsl_create_with_host_comm(ctypes.byref(protocol.desc()), ctypes.byref(cfg),
                                               ctypes.byref(host_comm.struct), ctypes.byref(handle))
            check(rc, "dsl_create_with_host_comm")
        else:
            check(lib.dsl_create(ctypes.byref(protocol.desc()), ctypes.byref(cfg), ctypes.byref(handle)),
                  "dsl_create")
        self.handle = handle

    def close(self):
        if self.handle:
            self.lib.dsl_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def state_bytes(self) -> int:
        return self.lib.dsl_state_bytes(ctypes.byref(self.protocol.desc()))

    def initial_packed(self) -> bytes:
        n = self.state_bytes()
        buf = (ctypes.c_uint8 * n)()
        check(self.lib.dsl_get_initial(self.handle, buf, n), "dsl_get_initial")
        return bytes(buf)

    def kernel_stats(self) -> dict:
        st = _lib.dsl_stats()
        check(self.lib.dsl_kernel_stats(self.handle, ctypes.byref(st)), "dsl_kernel_stats")
        return {name: getattr(st, name) for name, _ in st._fields_}

    def _prepare(self, state: SearchState, settings: SearchSettings):
        lib = self.lib
        enc = settings._encode(state)
        # the watches: told to the engine only when they differ from what it holds (a search without
        # watches on an engine without them makes no call). Watches the new settings do not have
        # leave first, so the new settings are never refused for the old watches' share of the
        # programs; the new ones follow the settings.
        wenc = settings._encode_watches(state)
        held = getattr(self, "_set_watch_key", b"")
        if wenc[0] != held and held:
            check(lib.dsl_set_watches(self.handle, None, 0, None, 0), "dsl_set_watches")
            self._set_watch_key = held = b""
            self._set_witness_mask = 0  # dsl_set_watches resets it
        # the step invariants: as the watches, told only when they differ from what the engine holds,
        # the old ones leaving before the new settings arrive
        senc = settings._encode_steps(state)
        sheld = getattr(self, "_set_step_key", b"")
        if senc[0] != sheld and sheld:
            check(lib.dsl_set_step_invariants(self.handle, None, 0, None, 0), "dsl_set_step_invariants")
            self._set_step_key = sheld = b""
        if enc is not getattr(self, "_set_enc", None):  # the engine keeps the settings it was given
            check(lib.dsl_set_settings(self.handle, ctypes.byref(enc)), "dsl_set_settings")
            self._set_enc = enc
            self._set_dropped = None  # dsl_set_settings re-applies the dropped set the engine holds
        if wenc[0] != held:
            check(lib.dsl_set_watches(self.handle, wenc[1], wenc[2], wenc[3], wenc[4]), "dsl_set_watches")
            self._set_watch_key = wenc[0]
            self._set_witness_mask = 0
        # the witness requests: only with watches, and only when they differ from what the engine holds
        if settings._watches and settings._witness_mask() != getattr(self, "_set_witness_mask", 0):
            check(lib.dsl_set_watch_witnesses(self.handle, settings._witness_mask()), "dsl_set_watch_witnesses")
            self._set_witness_mask = settings._witness_mask()
        if senc[0] != sheld:
            check(lib.dsl_set_step_invariants(self.handle, senc[1], senc[2], senc[3], senc[4]), "dsl_set_step_invariants")
            self._set_step_key = senc[0]
        # the event census: told only when it differs from what the engine holds
        if settings._event_census != getattr(self, "_set_event_census", False):
            check(lib.dsl_set_event_census(self.handle, int(settings._event_census)), "dsl_set_event_census")
            self._set_event_census = settings._event_census
        if state.packed is not None:
            buf = (ctypes.c_uint8 * len(state.packed)).from_buffer_copy(state.packed)
            check(lib.dsl_set_initial(self.handle, buf, len(state.packed), state.depth()), "dsl_set_initial")
        # the dropped network: part of network() for network predicates (SearchState.java:153-157)
        dr = tuple(state._dropped)
        if dr != getattr(self, "_set_dropped", None):
            arr = (ctypes.c_uint64 * max(1, len(dr)))(*dr)
            check(lib.dsl_set_dropped(self.handle, arr, len(dr)), "dsl_set_dropped")
            self._set_dropped = dr

    def bfs(self, state: SearchState, settings: Optional[SearchSettings] = None) -> SearchResults:
        if settings is None:
            settings = SearchSettings()
        self._prepare(state, settings)
        res_p = ctypes.POINTER(_lib.dsl_result)()
        check(self.lib.dsl_run(self.handle, ctypes.byref(res_p)), "dsl_run")
        res = self._results(state, settings, res_p)
        for w in range(len(settings._watches)):  # the census of this run (dsl_watch_counts)
            n, total = ctypes.c_int32(0), ctypes.c_uint64(0)
            buf = (ctypes.c_uint64 * max(1, len(res.per_depth)))()
            check(self.lib.dsl_watch_counts(self.handle, w, buf, len(res.per_depth), ctypes.byref(n),
                                            ctypes.byref(total)), "dsl_watch_counts")
            res._watch_counts.append([buf[i] for i in range(min(n.value, len(res.per_depth)))])
            res._watch_totals.append(total.value)
        if settings._event_census:  # the event census of this run (dsl_event_census)
            n = ctypes.c_int32(0)
            check(self.lib.dsl_event_census(self.handle, 0, None, ctypes.byref(n)), "dsl_event_census")
            ncls, nn = len(self.protocol.event_classes()), len(self.protocol.addresses)
            cells = (_lib.dsl_event_count * (_lib.DSL_EVENT_CLASSES * _lib.DSL_EVENT_NODES))()
            for lev in range(n.value):
                check(self.lib.dsl_event_census(self.handle, lev, cells, None), "dsl_event_census")
                res._event_rows.append([[(x.events, x.noops, x.exceptions, x.fresh)
                                         for x in cells[c * _lib.DSL_EVENT_NODES:c * _lib.DSL_EVENT_NODES + nn]]
                                        for c in range(ncls)])
            res._event_classes = self.protocol.event_classes()
            res._event_addresses = list(self.protocol.addresses)
        if settings._step_invariants:  # the step invariants' edge rows and violation of this run
            n, total = ctypes.c_int32(0), ctypes.c_uint64(0)
            buf = (ctypes.c_uint64 * max(1, len(res.per_depth)))()
            check(self.lib.dsl_step_edges(self.handle, buf, len(res.per_depth), ctypes.byref(n), ctypes.byref(total)),
                  "dsl_step_edges")
            res._step_edges = [buf[i] for i in range(min(n.value, len(res.per_depth)))]
            res._step_violation = self._step_violation_of(state, settings, len(res.per_depth) + 1)
            sv = res._step_violation
            if sv is not None and res._end == EndCondition.INVARIANT_VIOLATED and res._predicate is None:
                res._predicate = PredicateResult(_step_invariant(settings, sv.index), False)  # the reported terminal
        if any(settings._witness):  # the witnesses of this run (dsl_watch_witness)
            base = state.trace() if state.packed is not None else []
            nb = self.state_bytes()
            for w, want in enumerate(settings._witness):
                res._witnesses.append(self._witness_state(w, len(res.per_depth), nb, base, state._dropped) if want
                                      else None)
        return res

    def _step_violation_of(self, state: SearchState, settings: SearchSettings, cap: int) -> Optional[StepViolation]:
        nb = self.state_bytes()
        idx, depth, n, edges = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(0), ctypes.c_uint64(0)
        per = (ctypes.c_uint64 * _lib.DSL_MAX_STEP_INVARIANTS)()
        tr = (_lib.dsl_event * max(1, cap))()
        pbuf, xbuf = (ctypes.c_uint8 * nb)(), (ctypes.c_uint8 * nb)()
        check(self.lib.dsl_step_violation(self.handle, ctypes.byref(idx), ctypes.byref(depth), ctypes.byref(edges), per,
                                          tr, cap, ctypes.byref(n), pbuf, xbuf, nb), "dsl_step_violation")
        if idx.value < 0:
            return None
        raw = [_lib.dsl_event.from_buffer_copy(tr[i]) for i in range(min(n.value, cap))]
        base = state.trace() if state.packed is not None else []
        ev = [self.protocol.render_event(e) for e in raw]
        parent = SearchState(self.protocol, bytes(pbuf), depth.value - 1, base + ev[:-1], raw[:-1], state._dropped)
        succ = SearchState(self.protocol, bytes(xbuf), depth.value, base + ev, raw, state._dropped)
        return StepViolation(idx.value, settings._step_invariants[idx.value].name, depth.value, parent, succ, ev[-1],
                             edges.value, [per[i] for i in range(len(settings._step_invariants))])

    def _witness_state(self, w: int, cap: int, nb: int, base: List[str], dropped) -> Optional[SearchState]:
        depth, n = ctypes.c_int32(-1), ctypes.c_int32(0)
        tr = (_lib.dsl_event * max(1, cap))()
        buf = (ctypes.c_uint8 * nb)()
        check(self.lib.dsl_watch_witness(self.handle, w, ctypes.byref(depth), tr, cap, ctypes.byref(n), buf, nb),
              "dsl_watch_witness")
        if depth.value < 0:
            return None
        raw = [_lib.dsl_event.from_buffer_copy(tr[i]) for i in range(min(n.value, cap))]
        return SearchState(self.protocol, bytes(buf), depth.value, base + [self.protocol.render_event(e) for e in raw],
                           raw, dropped)

    def dfs(self, state: SearchState, settings: Optional[SearchSettings] = None, probes: int = 65536,
            seed: int = 0, max_probes: int = 0, minimize: bool = True, max_trace: int = 0) -> SearchResults:
        """Search.dfs / RandomDFS (Search.java:397-402, :507-583) on the device: `probes` random
        walks at once until a terminal state, settings.maxTimeSecs, or `max_probes` probes. The
        terminal's trace is minimized as RandomDFS does (TraceMinimizer) unless minimize=False."""
        if settings is None:
            settings = SearchSettings()
        self._prepare(state, settings)
        c = _lib.dsl_dfs_config(probes, seed & ((1 << 64) - 1), max_probes, 0, max_trace, 0 if minimize else 1, 0)
        res_p = ctypes.POINTER(_lib.dsl_result)()
        check(self.lib.dsl_run_dfs(self.handle, ctypes.byref(c), ctypes.byref(res_p)), "dsl_run_dfs")
        return self._results(state, settings, res_p)

    def replay(self, state: SearchState, settings: Optional[SearchSettings], events,
               minimize: bool = True) -> SearchResults:
        """TraceReplaySearch (T/junit/TraceReplaySearch.java:76-101): replays `events` (dsl_event
        list, e.g. ``SearchState.events()`` of an earlier result from the same start state) with
        checkState after every step; a terminal is minimized (TraceMinimizer) when `minimize`. An
        event that cannot be delivered, or the end of the trace, ends with SPACE_EXHAUSTED."""
        if settings is None:
            settings = SearchSettings()
        self._prepare(state, settings)
        arr = (_lib.dsl_event * max(1, len(events)))()
        for i, e in enumerate(events):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(e), ctypes.sizeof(_lib.dsl_event))
        res_p = ctypes.POINTER(_lib.dsl_result)()
        check(self.lib.dsl_replay(self.handle, arr, len(events), 1 if minimize else 0, ctypes.byref(res_p)),
              "dsl_replay")
        return self._results(state, settings, res_p)

    def human_readable_trace(self, state: SearchState, settings: Optional[SearchSettings], events) -> SearchState:
        """SearchState.humanReadableTraceEndState (SearchState.java:373-470): the state reached by
        `events` from `state`, whose trace() is the causally reordered, no-op-free trace."""
        if settings is None:
            settings = SearchSettings()
        self._prepare(state, settings)
        arr = (_lib.dsl_event * max(1, len(events)))()
        for i, e in enumerate(events):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(e), ctypes.sizeof(_lib.dsl_event))
        res_p = ctypes.POINTER(_lib.dsl_result)()
        check(self.lib.dsl_human_readable_trace(self.handle, arr, len(events), ctypes.byref(res_p)),
              "dsl_human_readable_trace")
        try:
            r = res_p.contents
            raw = [r.trace[i] for i in range(r.trace_len)]
            packed = bytes(ctypes.cast(r.terminal_state, ctypes.POINTER(ctypes.c_uint8 * r.state_bytes)).contents)
            return SearchState(self.protocol, packed, r.terminal_depth, [self.protocol.render_event(e) for e in raw],
                               [_lib.dsl_event.from_buffer_copy(e) for e in raw], state._dropped)
        finally:
            self.lib.dsl_result_free(res_p)

    def _results(self, state: SearchState, settings: SearchSettings, res_p) -> SearchResults:
        lib = self.lib
        try:
            r = res_p.contents
            per_depth = [r.per_depth[i] for i in range(r.n_levels)]
            end = EndCondition(r.end_condition)
            terminal = None
            last = None
            pred = None
            if r.terminal_state:
                raw = [r.trace[i] for i in range(r.trace_len)]
                events = [self.protocol.render_event(e) for e in raw]
                packed = bytes(ctypes.cast(r.terminal_state, ctypes.POINTER(ctypes.c_uint8 * r.state_bytes)).contents)
                base_events = state.trace() if state.packed is not None else []
                last = SearchState(self.protocol, packed, r.terminal_depth if r.terminal_depth >= 0 else r.max_depth,
                                   base_events + events, [_lib.dsl_event.from_buffer_copy(e) for e in raw],
                                   state._dropped)
                if r.terminal_depth >= 0:
                    terminal = last
                if end == EndCondition.INVARIANT_VIOLATED:
                    ninv = len(settings._invariants)  # past them: a step invariant (Engine.bfs names it)
                    pred = PredicateResult(settings.invariants()[r.predicate_index], False) \
                        if r.predicate_index < ninv else None
                elif end == EndCondition.GOAL_FOUND:
                    pred = PredicateResult(settings.goals()[r.predicate_index], True)
            res = SearchResults(end, r.states, per_depth, r.initial_depth, r.max_depth, terminal, pred,
                                r.elapsed_s, r.successors)
            res._last = last
            res._terminals_total = r.terminals_total
            base = state.trace() if state.packed is not None else []
            for i in range(r.n_terminals):
                t = r.terminals[i]
                t_end = EndCondition(t.end_condition)
                t_raw = [t.trace[j] for j in range(t.trace_len)]
                t_state = SearchState(
                    self.protocol, bytes(ctypes.cast(t.state, ctypes.POINTER(ctypes.c_uint8 * r.state_bytes)).contents),
                    r.terminal_depth, base + [self.protocol.render_event(e) for e in t_raw],
                    [_lib.dsl_event.from_buffer_copy(e) for e in t_raw], state._dropped)
                t_pred = None
                if t_end == EndCondition.INVARIANT_VIOLATED:
                    t_pred = PredicateResult(_step_invariant(settings, t.predicate_index - len(settings._invariants)), False) \
                        if t.predicate_index >= len(settings._invariants) else \
                        PredicateResult(settings.invariants()[t.predicate_index], False)
                elif t_end == EndCondition.GOAL_FOUND:
                    t_pred = PredicateResult(settings.goals()[t.predicate_index], True)
                res._terminals.append((t_end, t_pred, t_state))
            # CheckLogger.notDeterministic / notIdempotent (T/utils/CheckLogger.java:104-121)
            res.checks = {"run": r.checks_run, "not_deterministic": r.not_deterministic,
                          "not_idempotent": r.not_idempotent,
                          "first_not_deterministic": self.protocol.render_event(r.first_not_deterministic)
                          if r.not_deterministic else None,
                          "first_not_idempotent": self.protocol.render_event(r.first_not_idempotent)
                          if r.not_idempotent else None}
            return res
        finally:
            lib.dsl_result_free(res_p)


def _step_invariant(settings: SearchSettings, index: int) -> StatePredicate:
    """Step invariant ``index`` of the settings."""
    return settings._step_invariants[index]


class Search:
    @staticmethod
    def bfs(initialState: SearchState, settings: Optional[SearchSettings] = None, device: int = -1) -> SearchResults:
        """Search.bfs (Search.java:390-395) on the MI355X engine."""
        eng = Engine(initialState.protocol, device=device)
        try:
            return eng.bfs(initialState, settings)
        finally:
            eng.close()

    @staticmethod
    def replay(initialState: SearchState, settings: Optional[SearchSettings], events, minimize: bool = True,
               device: int = -1) -> SearchResults:
        """TraceReplaySearch on the MI355X engine's transitions (host side, see Engine.replay)."""
        eng = Engine(initialState.protocol, device=device)
        try:
            return eng.replay(initialState, settings, events, minimize)
        finally:
            eng.close()

    @staticmethod
    def dfs(initialState: SearchState, settings: Optional[SearchSettings] = None, device: int = -1,
            **kw) -> SearchResults:
        """Search.dfs (Search.java:397-402): random depth-first probes on the MI355X engine."""
        eng = Engine(initialState.protocol, device=device)
        try:
            return eng.dfs(initialState, settings, **kw)
        finally:
            eng.close()
