"""synth_fast (what bench.py generates its pictures with) must give the bytes of synth, the generator the reference
digests were recorded on."""
import pytest

from synth import synth, synth_fast


@pytest.mark.parametrize("w,h,cf,bits,seed,frames,wb", [(64, 32, "422", 10, 3, 2, 2), (96, 48, "420", 8, 5, 3, 1),
                                                        (80, 40, "444", 12, 7, 2, 2), (3840, 2160, "422", 10, 1234, 1, 2)])
def test_synth_fast_is_synth(w, h, cf, bits, seed, frames, wb):
    assert synth_fast(w, h, cf, bits, seed, frames=frames, word_bytes=wb) == synth(w, h, cf, bits, seed, frames=frames, word_bytes=wb)

