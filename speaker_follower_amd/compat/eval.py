"""`import eval` (train.py:17; `eval.Evaluation([split])`, train.py:206) / `from eval import Evaluation` (plot.py:7)."""
from speaker_follower_amd.evaluation import Evaluation, EvalResult      # noqa: F401
from speaker_follower_amd.evaluation import PathEvalResult, path_metrics_of      # noqa: F401
from speaker_follower_amd.evaluation import CoverageEvalResult, coverage_metrics_of      # noqa: F401
from speaker_follower_amd.evaluation import eval_simple_agents, evaluate_simple_agents      # noqa: F401  (eval.py:148-163)
