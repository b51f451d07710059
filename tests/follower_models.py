"""The follower's encoder and decoder at the `synth.FULL` dimensions with seeded peaky weights, on the GPU in eval mode
(tests/test_gpu_text_fold.py, tests/test_gpu_decode_schedules.py: the folded decode chains only engage at these sizes)."""
import torch

from speaker_follower_amd import synth


def full_size_models(seed=77):
    from speaker_follower_amd import model
    d = synth.FULL
    enc_w, dec_w = synth.follower_weights_peaky(seed)
    enc = model.EncoderLSTM(d.vocab, d.word, d.hidden, 0, 0.5, glove=enc_w['embedding.weight'])
    dec = model.AttnDecoderLSTM(d.feat, d.hidden, 0.5, feature_size=d.feat)
    enc.load_state_dict({k: torch.tensor(v) for k, v in enc_w.items()})
    dec.load_state_dict({k: torch.tensor(v) for k, v in dec_w.items()})
    return enc.cuda().eval(), dec.cuda().eval(), enc_w, dec_w
