"""`import eval_speaker` (train_speaker.py:17; `eval_speaker.SpeakerEvaluation([split], ...)`, train_speaker.py:199;
rational_speaker.py, validate_speaker.py, data_augmentation_from_speaker.py).  `SpeakerEvaluation(...,
caption_metrics=True)` adds ROUGE-L and CIDEr-D to the summary; their parts and the one function that forms them are
exported beside it."""
from speaker_follower_amd.speaker_evaluation import SpeakerEvaluation      # noqa: F401
from speaker_follower_amd.speaker_evaluation import (caption_corpus, caption_parts_rows, caption_scores_of,  # noqa: F401
                                                     caption_static_rows)
