"""Foreign streams through the device's submission layer (kvazzup_amd/csrc/batch.h, batch.hip; the _n kernels of dec_kernels.hip): whenever more than one decoder is
open on a device -- every call with several peers -- no decoder launches its own pictures, and what the layer decides exists on that path alone: one form of the
intra chain for a whole launch (a plain picture beside a general one runs the general form), workgroups shared out from every picture's own geometry and padded
to 8 (a 24x16 picture: one workgroup, seven of padding; coding tree blocks of 32 and 16 samples: cwc != wc), pictures with constrained intra prediction that
hop between the layer and their decoder's own launches, concealment that drains the device beside other decoders' batches, a peer that joins a decoder running
alone on two chains, and the batch limit of eight.  tests/test_gpu_batch.py runs the layer on the checker's own encoder's streams only; here B pictures, explicit
weights, list modification, the CTB and minimum coding block sizes, free slices, tile grids with closed filter boundaries, PCM, constrained intra prediction,
scaling lists, transquant bypass, long-term references and lost pictures under both concealment modes share launches.  Every decoder's pictures must be the
checker's (the model decoder's in mode 3) bit for bit: deckit.together.  The streams and what each brings: tests/batch_cases.py, held to that on the CPU by
tests/test_batch_foreign_cases.py."""
import pytest

import batch_cases as bc
from deckit import together


@pytest.mark.gpu
def test_eight_forms_in_one_launch(gpu):
    """held, the eight first pictures leave together: that one intra launch mixes plain and general pictures, CTBs of 64, 32 and 16 samples and a picture of one
    workgroup; the later launches B, P and I pictures with and without SAO, weights and scaling lists"""
    streams = bc.eight_forms()
    st = together(streams, hold=True)
    assert st["sizes"][8] >= 1, st
    assert st["pictures"] == bc.total(streams), st


@pytest.mark.gpu
def test_more_decoders_than_a_batch_holds(gpu):
    """ten decoders: two first pictures stay behind for the next batch, beside six second ones; nothing is lost or launched twice"""
    streams = bc.ten_decoders()
    st = together(streams, hold=True)
    assert st["sizes"][8] >= 1, st
    assert st["pictures"] == bc.total(streams), st


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
def test_constrained_intra_prediction_hops_between_the_layer_and_its_own_launches(gpu, hold):
    """a picture with constrained intra prediction and both kinds of block has no batched form: its decoder launches it itself, behind what it still has queued in the
    layer (DecBatcher::drain) and on the same stream; the pictures around it go through the layer beside the other decoders'.  Held, the decoder's own launch
    waits in drain behind held pictures."""
    streams = bc.cip_hop()
    st = together(streams, hold=hold)
    assert st["pictures"] == bc.total(streams) - streams[0]["mixed"], (st, streams[0]["kinds"])


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(12))
def test_everything_at_once_together(gpu, group):
    """the 48 draws of tests/test_gpu_everything.py four at a time, synchronous and frame-threaded decoders side by side; every other group in full batches"""
    st = together(bc.everything(group), hold=bool(group & 1))
    assert st["pictures"] > 0, st


@pytest.mark.gpu
def test_lost_pictures_beside_other_decoders(gpu):
    """three decoders fill stand-ins for lost reference pictures -- each waits for its own queued pictures and drains the device while the others' batches are in
    flight; mode 3 launches its kernel on the shared stream -- beside one that decodes a clean stream"""
    together(bc.lost_pictures())


@pytest.mark.gpu
def test_a_peer_joins_and_leaves(gpu):
    """a frame-threaded decoder on all-intra pictures alternates its two chains while it is alone; a second decoder opens (the second chain's pictures first, then
    the layer), closes, a third one opens and closes: the first changes path in order every time.  (With four frame threads handing in access unit k launches
    picture k - 1, Decoder::submit_job's "pipeline still filling": by its third access unit the first decoder has launched two pictures itself, one on each
    chain, so the peer finds the second chain in use and fewer than all pictures reach the layer.)"""
    streams = bc.join_and_leave()
    st = together(streams)
    assert 0 < st["pictures"] < bc.total(streams), st
