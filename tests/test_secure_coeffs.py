"""The pure-Python coefficient helper of tests/test_gpu_secure_batch.py (tests/secure_coeffs.py) reproduces SURVEY Appendix A:
H and t for the reference's two- and three-key test vectors, Modern and Legacy."""
import json
import os

import util
from secure_coeffs import R, secure_coefficients, aggregate_secret

KATS = json.load(open(os.path.join(util.ROOT, 'tests', 'golden', 'ref_kats.json')))
PK = [bytes.fromhex(h) for h in KATS['cpp']['pk']]


def test_modern_rows():
    order, H, ts = secure_coefficients(PK[:2])
    assert order == [1, 0]
    assert H.hex() == '6040b788e954eb9df1a0d581cf020f7b1946d0ed0dd48de1d03bab45e3b3a29a'
    assert [ts[i] for i in order] == [0x584ccd89aaf51f8b06067b165b36a9096ae4abc23189c97ca1d34accb015244a,
                                      0x350f133013a3e8f028ab28c14c710b88cc15bfaa853497887728fe591c20a17d]
    order, H, ts = secure_coefficients(PK)
    assert order == [2, 1, 0]
    assert H.hex() == '2bea60d6e626726b25830ee4fbc3c51039b360c5c1005712cc5e1bb3aece7b9b'
    assert [ts[i] for i in order] == [0x06affd8cb2dc37f9c3c4b15a8e7dc6c9b12a845877d24eaa2e2be6628dda7755,
                                      0x5bcd568774ca9fbe351d45b43e504a2f17d6d169142a4286414e90a9de5b01a8,
                                      0x07a4139aa0177dbc814d996431d547dca201ca30ff948d57c7d40bfed02f3c9e]


def test_legacy_rows():
    leg = [util.ref.modern_to_legacy(b) for b in PK]
    order, H, ts = secure_coefficients(leg[:2])
    assert order == [1, 0]
    assert H.hex() == 'e071762f006645a6561b37e91663c569561a2a8a26abe1b883cc9b0810418107'
    assert [ts[i] for i in order] == [0x110b46124e620f32454766cab9cbb21839f426d69acb9053b9d34b18475d9cb5,
                                      0x46137f35eff8efc8910a117a3bdc58c3c0aa7cbb16d53a1f6987261b16b5755e]
    order, H, ts = secure_coefficients(leg)
    assert order == [2, 1, 0]
    assert H.hex() == '88ec5f152a807e8f64a0639972defc88caa305a548fe290897e27ef2a052f140'
    assert [ts[i] for i in order] == [0x43cc66d4a23309b3e0d7c75dc3d2d04df70e6f9f6d826b025ecaf81371906b00,
                                      0x6fbe54b6d98e29d8e2edad9e0962a4070690d74ab1b9425f154f990dd64c793c,
                                      0x48b0c8fe31dde82cb08bb7666233296901c34e121f19653d3b238ade1a5d971c]


def test_stable_order_and_secret():
    """Duplicates keep their input order (Rust's sort_by is stable); the aggregate secret is sum t_i k_i mod r."""
    kb = [b'\x02' * 48, b'\x01' * 48, b'\x02' * 48, b'\x01' * 48]
    order, _, ts = secure_coefficients(kb)
    assert order == [1, 3, 0, 2]
    assert all(0 <= t < R for t in ts)
    assert aggregate_secret(kb, [1, 0, 0, 0]) == ts[0]
    assert aggregate_secret(kb, [2, 3, 0, 1]) == (2 * ts[0] + 3 * ts[1] + ts[3]) % R
