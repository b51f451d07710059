"""`import eval_speaker` (train_speaker.py:17; `eval_speaker.SpeakerEvaluation([split], ...)`, train_speaker.py:199;
rational_speaker.py, validate_speaker.py, data_augmentation_from_speaker.py)."""
from speaker_follower_amd.speaker_evaluation import SpeakerEvaluation      # noqa: F401
