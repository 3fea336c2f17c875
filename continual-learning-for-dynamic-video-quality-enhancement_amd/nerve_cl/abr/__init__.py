"""ABR (adaptive bitrate) components: the streaming environment (host and vectorised on the device) and the PPO agent."""
from nerve_cl.abr.environment import StreamingEnv, VecStreamingEnv, QualityLevel, make_env
from nerve_cl.abr.agent import PPOAgent, ActorCritic, ABRConfig

__all__ = ["StreamingEnv", "VecStreamingEnv", "QualityLevel", "make_env", "PPOAgent", "ActorCritic", "ABRConfig"]
