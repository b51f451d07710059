"""`from bleu import multi_bleu` (eval_speaker.py:8, rational_speaker.py): no perl, no temporary files."""
from speaker_follower_amd.speaker_evaluation import multi_bleu, single_bleu      # noqa: F401
