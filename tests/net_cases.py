"""pb.json restated with user-written message predicates (MessagePattern.where, DSL_PRED_NET), shared
by the CPU-baseline and the engine tests: every `hasViewReply:N` / `hasViewReply:N:P:B` of a case,
alone or inside and(...) / !, becomes the generic network leaf over PBIR's ViewReply record;
`viewRepliesSent` (it compares a record field with a node field) and every other name stay as they
are. Every expected value comes from the committed fixture (written by the oracle with the NAMED
predicates), never from the code under test."""
import json
import os

import argmap
from dslabs_amd.protocols import PBIR

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "pb.json")) as _f:
    GOLD = json.load(_f)


def has_view_reply(proto, n, p=None, b=None):
    """PrimaryBackupTest.hasViewReply(n) (viewNum >= n) or hasViewReply(n, p, b) (exactly
    View(n, p, b); p and b are server numbers, -1 = null, which the record holds as 0)."""
    vr = proto.message("ViewReply")
    if p is None:
        return vr.where(vr.field("num") >= n)
    return vr.where(vr.field("num") == n, vr.field("p") == max(p, 0), vr.field("b") == max(b, 0))


class Restated:
    """What argmap.predicate asks a protocol for, with the hasViewReply names restated."""

    def __init__(self, proto):
        self.proto = proto

    def predicate(self, name):
        if name.startswith("hasViewReply:"):
            return has_view_reply(self.proto, *[int(x) for x in name.split(":")[1:]])
        return self.proto.predicate(name)


def uses_has_view_reply(case) -> bool:
    return any("hasViewReply:" in a for a in case["args"])


CASES = sorted(n for n, c in GOLD.items() if isinstance(c, dict) and "args" in c and uses_has_view_reply(c))


def case(name, restated=True, table_log2=20):
    """(fixture, PBIR, settings) of a pb.json case; restated=False keeps the named predicates."""
    gold = GOLD[name]
    args = ["pb_ir" if a == "pb" else a for a in gold["args"]]
    proto = argmap.protocol(args)
    assert isinstance(proto, PBIR)
    settings = argmap.settings(args, Restated(proto) if restated else proto, table_log2=table_log2)
    return gold, proto, settings
