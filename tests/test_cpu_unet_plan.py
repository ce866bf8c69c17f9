"""The forward plan of a conv + BatchNorm + ReLU layer (``unet_ops._forward_plan``) over every combination of its six boolean inputs,
against a literal table: which statistics path the layer takes, whether the stem kernels serve it, and whether room for an accumulator
is claimed in the step block -- only where the accumulator path is otherwise reached."""
import itertools

# training, stem-capable, counter available, _BN_ACC and not float statistics, fwd_acc_supported, accumulator obtained
#   -> path, stem kernels, accumulator requested
TABLE = """
    000000 eval    0 0
    000001 eval    0 0
    000010 eval    0 0
    000011 eval    0 0
    000100 eval    0 0
    000101 eval    0 0
    000110 eval    0 0
    000111 eval    0 0
    001000 eval    0 0
    001001 eval    0 0
    001010 eval    0 0
    001011 eval    0 0
    001100 eval    0 0
    001101 eval    0 0
    001110 eval    0 0
    001111 eval    0 0
    010000 eval    1 0
    010001 eval    1 0
    010010 eval    1 0
    010011 eval    1 0
    010100 eval    1 0
    010101 eval    1 0
    010110 eval    1 0
    010111 eval    1 0
    011000 eval    1 0
    011001 eval    1 0
    011010 eval    1 0
    011011 eval    1 0
    011100 eval    1 0
    011101 eval    1 0
    011110 eval    1 0
    011111 eval    1 0
    100000 rows    0 0
    100001 rows    0 0
    100010 rows    0 0
    100011 rows    0 0
    100100 rows    0 0
    100101 rows    0 0
    100110 rows    0 1
    100111 acc     0 1
    101000 counter 0 0
    101001 counter 0 0
    101010 counter 0 0
    101011 counter 0 0
    101100 counter 0 0
    101101 counter 0 0
    101110 counter 0 0
    101111 counter 0 0
    110000 rows    0 0
    110001 rows    0 0
    110010 rows    0 0
    110011 rows    0 0
    110100 rows    0 1
    110101 acc     1 1
    110110 rows    0 1
    110111 acc     1 1
    111000 counter 0 0
    111001 counter 0 0
    111010 counter 0 0
    111011 counter 0 0
    111100 counter 0 0
    111101 counter 0 0
    111110 counter 0 0
    111111 counter 0 0
"""

WORDS = 34


class _Block:
    """A step block that has room for the accumulator, or has none left."""

    def __init__(self, room: bool):
        self.room, self.requests, self.words = room, [], object()

    def acc64(self, n):
        self.requests.append(n)
        return self.words if self.room else None


def test_forward_plan_over_all_inputs():
    from miseg_amd import unet_ops
    rows = [line.split() for line in TABLE.strip().splitlines()]
    assert [r[0] for r in rows] == ["".join(map(str, bits)) for bits in itertools.product((0, 1), repeat=6)]
    for bits, want_path, want_stem, want_request in rows:
        training, stem_ok, counter_ok, use_acc, acc_supported, obtained = (b == "1" for b in bits)
        io = _Block(obtained)
        path, stem, acc = unet_ops._forward_plan(training, stem_ok, counter_ok, use_acc, acc_supported, io, WORDS)
        assert (path, stem, len(io.requests)) == (want_path, want_stem == "1", int(want_request)), bits
        assert io.requests in ([], [WORDS]), bits
        assert acc is (io.words if path == "acc" else None), bits


def test_forward_plan_without_a_step_block():
    """Stand-alone use of the layer: the accumulator path wherever it is reached, with an accumulator the caller zero-fills."""
    from miseg_amd import unet_ops
    for training, stem_ok, counter_ok, use_acc, acc_supported in itertools.product((False, True), repeat=5):
        with_room = unet_ops._forward_plan(training, stem_ok, counter_ok, use_acc, acc_supported, _Block(True), WORDS)
        alone = unet_ops._forward_plan(training, stem_ok, counter_ok, use_acc, acc_supported, None, WORDS)
        assert alone == (with_room[0], with_room[1], None)
