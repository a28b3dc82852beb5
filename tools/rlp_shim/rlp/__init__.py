"""Minimal stand-in for the `rlp` package, enough for the reference's `state`
package to import and run (tools/gen_state_proofs_golden.py only): encode /
decode of nested byte strings, codec.encode_raw, and the sedes names
state/util/utils.py touches at import time.  decode is strict about lengths
(an item that overruns its parent, or bytes after the top-level item, raise
DecodingError), as the real package is."""
from . import codec, sedes  # noqa: F401
from .codec import DecodingError, decode, encode  # noqa: F401
