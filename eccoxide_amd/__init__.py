"""eccoxide_amd -- MI355X-native batched scalar multiplication behind eccoxide's
CurveGroup / Point / Scalar surface (hot path only)."""
from .engine import (  # noqa: F401
    BLS12_381_G1, BLS12_381_G2, CURVE_IDS, CURVE_NAMES, ED25519, FLAG_FINITE, FLAG_INFINITY, FLAG_REJECTED, JUBJUB, P256R1, P384R1,
    P521R1, P256K1, PAIRING_NOT_ONE, PAIRING_ONE, PAIRING_REJECTED, SIG_BAD_KEY, SIG_INVALID, SIG_MALFORMED, SIG_VALID, SIGN_NONE, SIGN_OK, EccxError, Engine, curve_id, field_bytes,
    scalar_bytes,
)
