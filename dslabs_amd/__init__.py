"""dslabs_amd: MI355X-native breadth-first model checking for DSLabs protocols.

The product is ``libdslabs_hip.so`` (HIP kernels for gfx950 behind the C ABI in
include/dslabs_hip.h); this package is the thin host-side mirror of the reference's
``Search`` / ``SearchSettings`` / ``SearchResults`` API over it.
"""
from .search import (CLIENTS_DONE, NONE_DECIDED, RESULTS_OK, EndCondition, Engine, EventCount, FieldRef,  # noqa: F401
                     MessagePattern, PredicateResult, Search, SearchResults, SearchSettings, SearchState, StatePredicate, allOf,
                     anyOf, clientDone, clientHasResults, field_value, message_matches, new, old, statePredicate,
                     StepFieldRef, StepViolation)

__all__ = ["Search", "SearchSettings", "SearchState", "SearchResults", "EndCondition", "StatePredicate",
           "PredicateResult", "Engine", "RESULTS_OK", "CLIENTS_DONE", "NONE_DECIDED", "clientDone",
           "clientHasResults", "FieldRef", "statePredicate", "allOf", "anyOf", "field_value", "MessagePattern",
           "message_matches", "EventCount", "old", "new", "StepFieldRef", "StepViolation"]
